// colate_amd/csrc/walk_resident.hpp -- what the device drivers over the pair walk share (interval_device.cpp: the interval fit;
// fill_samples_kernel.hip: the table fill of `--mode mut --samples`): the stream guard, the event timer, and the walk's inputs
// resident on the device with the count pass over them.  Host code for translation units compiled as HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "device_stage.hpp"
#include "em_job.hpp"
#include "interval_walk.h"

namespace colate_iw {

// Synchronises on scope exit.  Declared behind every host array that an asynchronous copy reads or writes and behind the
// DeviceBuffers of the scope, so that nothing the stream still uses is freed before the stream is idle -- also on an early return.
struct StreamSync {
  hipStream_t s;
  ~StreamSync() { (void)hipStreamSynchronize(s); }
};

// asynchronous host-to-device copy; nothing is enqueued for zero bytes
inline hipError_t h2d(hipStream_t stream, void* dst, const void* src, size_t bytes) {
  return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
}

// Pairs of events on a stream around the kernels of a call, for the *_kernel_seconds diagnostics: mark() opens and closes
// an interval in turn; seconds() sums them once the stream is idle; the events go on scope exit.
struct KernelTimer {
  hipStream_t stream;
  std::vector<hipEvent_t> ev;
  explicit KernelTimer(hipStream_t s) : stream(s) {}
  KernelTimer(const KernelTimer&) = delete;
  ~KernelTimer() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  hipError_t mark() {
    hipEvent_t e;
    if (hipError_t rc = hipEventCreate(&e)) return rc;
    ev.push_back(e);
    return hipEventRecord(e, stream);
  }
  double seconds() const {
    double s = 0.0;
    for (size_t i = 0; i + 1 < ev.size(); i += 2) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) s += ms * 1e-3;
    }
    return s;
  }
};

// The inputs of a view, resident on the device: uploaded once per call, chromosome by chromosome from where they lie.
struct Resident {
  colate::DeviceBuffers buf;
  DeviceInputs in;
  std::vector<long long> word_off;
  int upload(const View& v, hipStream_t stream) {
    const int C = v.C;
    in.C = C, in.S = v.S, in.M = v.M, in.P = v.P, in.nbpb = v.nbpb, in.n = v.row_off[C];
    word_off.resize((size_t)C + 1);
    in.words = mask_words(C, v.row_off, word_off.data());
    long long *d_row_off = nullptr, *d_word_off = nullptr;
    Row* d_rows = nullptr;
    Idx* d_idx = nullptr;
    unsigned long long* d_masks = nullptr;
    Pair* d_pairs = nullptr;
    HIP_TRY(buf.device(d_row_off, (size_t)C + 1)); HIP_TRY(buf.device(d_word_off, (size_t)C + 1));
    HIP_TRY(buf.device(d_rows, (size_t)in.n)); HIP_TRY(buf.device(d_idx, (size_t)v.S * in.n));
    HIP_TRY(buf.device(d_masks, (size_t)v.M * in.words)); HIP_TRY(buf.device(d_pairs, (size_t)v.P));
    HIP_TRY(h2d(stream, d_row_off, v.row_off, sizeof(long long) * ((size_t)C + 1)));
    HIP_TRY(h2d(stream, d_word_off, word_off.data(), sizeof(long long) * ((size_t)C + 1)));
    HIP_TRY(h2d(stream, d_pairs, v.pairs, sizeof(Pair) * (size_t)v.P));
    for (int c = 0; c < C; c++) {
      const size_t nc = (size_t)(v.row_off[c + 1] - v.row_off[c]), wc = (size_t)(word_off[(size_t)c + 1] - word_off[(size_t)c]);
      HIP_TRY(h2d(stream, d_rows + v.row_off[c], v.rows[c], sizeof(Row) * nc));
      for (int s = 0; s < v.S; s++) HIP_TRY(h2d(stream, d_idx + (size_t)s * in.n + v.row_off[c], v.idx[(size_t)s * C + c], sizeof(Idx) * nc));
      for (int m = 0; m < v.M; m++)
        HIP_TRY(h2d(stream, d_masks + (size_t)m * in.words + word_off[(size_t)c], v.masks[(size_t)m * C + c], sizeof(unsigned long long) * wc));
    }
    in.row_off = d_row_off, in.word_off = d_word_off, in.rows = d_rows, in.idx = d_idx, in.masks = d_masks, in.pairs = d_pairs;
    return COLATE_OK;
  }
  // The count pass for all pairs (timed) and the one host wait, for cnt / last [P][C]; from them every pair's first block per
  // chromosome blk0[P][C], its blocks nb[P] and the record offsets off[P + 1].
  std::vector<int> cnt, last, blk0, nb;
  std::vector<long long> off;
  int count(KernelTimer& timer) {
    const size_t PC = (size_t)in.P * in.C;
    int *d_cnt = nullptr, *d_last = nullptr;
    HIP_TRY(buf.device(d_cnt, PC)); HIP_TRY(buf.device(d_last, PC));
    HIP_TRY(timer.mark());
    if (hipError_t e = count_launch(in, 0, in.P, d_cnt, d_last, timer.stream)) return colate::hip_fail(e, "interval walk count kernel launch");
    HIP_TRY(timer.mark());
    cnt.resize(PC), last.resize(PC), blk0.resize(PC), nb.resize((size_t)in.P), off.resize((size_t)in.P + 1);
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * PC, hipMemcpyDeviceToHost, timer.stream));
    HIP_TRY(hipMemcpyAsync(last.data(), d_last, sizeof(int) * PC, hipMemcpyDeviceToHost, timer.stream));
    HIP_TRY(hipStreamSynchronize(timer.stream));
    return finish_counts(in.P, in.C, cnt.data(), last.data(), blk0.data(), nb.data(), off.data());
  }
};

}  // namespace colate_iw
