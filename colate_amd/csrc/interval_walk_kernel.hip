// colate_amd/csrc/interval_walk_kernel.hip -- the pair walk of `--mode mut_interval --samples` on the GPU (interval_walk.h:
// the walk contract, the record, the blocks; interval_walk.cpp: the host twin).
//
// ONE workgroup per (pair, chromosome) walks the chromosome's rows kTile at a time, thread t holding row base + t.  The
// walk's two states are "the latest row so far that the masks let through" and "the latest row so far that passed as
// reference"; what a row needs is the value of each in FRONT of it.  Within a wave that is the highest set bit below the
// lane in a ballot of the flag; in front of the wave it is the highest flagged row of the earlier waves of the tile (one
// int per wave through LDS) or else the carry from the earlier tiles, which every thread keeps alike in a register.
// Three such steps per tile, each closed by one barrier that every wave reaches (the loop runs over the tiles, which all
// threads count alike; ballots are taken with all 64 lanes active, a lane beyond the chromosome's end holding "no"):
//   1. pass  (masked pairs only; without masks the row in front is i - 1)      -> ref_from
//   2. passes as reference: r.DAF != 0 && r.prev_bp >= pos(ref_from)            -> tgt_from
//   3. used: (t.DAF | t.AAF) != 0 && t.prev_bp >= pos(tgt_from)                 -> rank among the used rows, and the used
//      row in front (its block decides which block ranges this row opens)
// Every LDS array is written in one step and read in the same step behind its barrier; the next write to it comes after
// the other barriers of the loop, so no buffer is reused before every wave has read it.
// The count pass keeps the number of used rows and the block of the last one; the write pass repeats the walk and writes
// record, block id and the block ranges at offsets the host formed from the counts between the two launches.  Integers
// only decide where anything goes; a workgroup reads nothing another workgroup of the same launch writes.
// The write pass has two forms of the same walk: the interval fit's record (make_rec), and for `--mode mut --samples` the record
// of the age-sampling kernel with its row-0 weights beside it (make_fill_rec; fill_samples_kernel.hip drives it).
#include <hip/hip_runtime.h>

#include "interval_walk.h"

using namespace colate_iw;
using colate_ic::IntervalRec;

namespace {

// where a used row goes in the write pass: the interval fit's record, or the table fill's record and its side entry
struct IntervalOut {
  IntervalRec* recs;
  __device__ __forceinline__ void put(long long at, const Row& m, const Idx& t, const Idx& r) const { recs[at] = make_rec(m, t, r); }
};
struct FillOut {
  colate_drv::FillRec* recs;
  FillSide* side;
  __device__ __forceinline__ void put(long long at, const Row& m, const Idx& t, const Idx& r) const {
    FillSide s;
    recs[at] = make_fill_rec(m, t, r, s);
    side[at] = s;
  }
};

struct Shared {
  int last[3][kWaves];  // per step and wave: the highest flagged row of the wave in this tile (-1: none)
  int count[kWaves];    // step 3: used rows of the wave
};

// mask: the ballot of a flag over this wave.  Returns the highest flagged row in front of this lane: within the wave, else
// the earlier waves', else the carry; `carry` becomes the highest flagged row up to the end of this tile.  One barrier.
__device__ __forceinline__ int latest_in_front(unsigned long long mask, int base, int wave, int lane, int* s_last, int& carry) {
  if (lane == 0) s_last[wave] = mask ? base + wave * 64 + (63 - __clzll((long long)mask)) : -1;
  __syncthreads();
  const unsigned long long prior = mask & ((1ull << lane) - 1ull);
  int from = carry, end = carry;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const int l = s_last[w];
    if (w < wave && l >= 0) from = l;  // (rows ascend with the wave: a later wave's entry is the higher row)
    if (l >= 0) end = l;
  }
  if (prior) from = base + wave * 64 + (63 - __clzll((long long)prior));
  carry = end;
  return from;
}

template <bool Masked, bool Write, class Out>
__device__ __forceinline__ void walk(Shared& s, int n, const Row* __restrict__ rows, const Idx* __restrict__ TI,
                                     const Idx* __restrict__ RI, const unsigned long long* __restrict__ tmask,
                                     const unsigned long long* __restrict__ rmask, int nbpb, int& out_count, int& out_last,
                                     long long rec0, int blk0, const Out out, int* __restrict__ block,
                                     long long* __restrict__ off_seg) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int searched = -1, ref_pass = -1, last_used = -1, count = 0;
  for (int base = 0; base < n; base += kTile) {
    const int i = base + tid;
    const bool in = i < n;
    // ---- 1. the row the reference cursor searched in front of this one
    int ref_from;
    bool pass = in;
    if (Masked) {
      if (in && tmask) pass = pass && ((tmask[i >> 6] >> (i & 63)) & 1ull);
      if (in && rmask) pass = pass && ((rmask[i >> 6] >> (i & 63)) & 1ull);
      ref_from = latest_in_front(__ballot(pass), base, wave, lane, s.last[0], searched);
    } else {
      ref_from = i - 1;
    }
    // ---- 2. passes as reference; the row the target cursor searched in front of this one
    Idx r{0, 0, 0};
    bool refp = false;
    if (pass) {
      r = RI[i];
      const int from_pos = ref_from < 0 ? -1 : rows[ref_from].pos;
      refp = r.DAF != 0 && r.prev_bp >= from_pos;
    }
    const int tgt_from = latest_in_front(__ballot(refp), base, wave, lane, s.last[1], ref_pass);
    // ---- 3. used; rank and the used row in front
    Idx t{0, 0, 0};
    bool used = false;
    if (refp) {
      t = TI[i];
      const int from_pos = tgt_from < 0 ? -1 : rows[tgt_from].pos;
      used = (t.DAF | t.AAF) != 0 && t.prev_bp >= from_pos;
    }
    const unsigned long long umask = __ballot(used);
    if (lane == 0) s.count[wave] = __popcll(umask);
    const int used_from = latest_in_front(umask, base, wave, lane, s.last[2], last_used);
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      const int c = s.count[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (Write && used) {
      const Row m = rows[i];
      const long long at = rec0 + count + before + __popcll(umask & ((1ull << lane) - 1ull));
      const int k = block_of_pos(m.pos, nbpb);
      out.put(at, m, t, r);
      if (block) block[at] = blk0 + k;
      if (off_seg) {  // the blocks this row opens: those behind the block of the used row in front of it, up to its own
        const int k_from = used_from < 0 ? -1 : block_of_pos(rows[used_from].pos, nbpb);
        for (int b = k_from + 1; b <= k; b++) off_seg[b] = at;
      }
    }
    count += total;
  }
  out_count = count;
  out_last = last_used;
}

template <bool Write, class Out>
__global__ __launch_bounds__(kTile) void interval_walk_kernel(DeviceInputs in, int p0, int* __restrict__ cnt,
                                                             int* __restrict__ last_block, const long long* __restrict__ rec0,
                                                             const int* __restrict__ blk0, const int* __restrict__ seg0,
                                                             const Out out, int* __restrict__ block,
                                                             long long* __restrict__ off, long long off_end, long long rec_end) {
  __shared__ Shared s;
  const int c = blockIdx.x % in.C, j = blockIdx.x / in.C;  // (pair p0 + j, chromosome c)
  const Pair pr = in.pairs[p0 + j];
  const long long r0 = in.row_off[c];
  const int n = (int)(in.row_off[c + 1] - r0);
  const Row* const rows = in.rows + r0;
  const Idx* const TI = in.idx + (size_t)pr.target * in.n + r0;
  const Idx* const RI = in.idx + (size_t)pr.reference * in.n + r0;
  const unsigned long long* const tmask = pr.target_mask < 0 ? nullptr : in.masks + (size_t)pr.target_mask * in.words + in.word_off[c];
  const unsigned long long* const rmask = pr.reference_mask < 0 ? nullptr : in.masks + (size_t)pr.reference_mask * in.words + in.word_off[c];
  const size_t slot = (size_t)j * in.C + c;
  long long my_rec0 = 0;
  int my_blk0 = 0;
  long long* off_seg = nullptr;
  if (Write) {
    my_rec0 = rec0[slot], my_blk0 = blk0[slot];
    if (off) off_seg = off + seg0[slot];
  }
  int count = 0, last = -1;
  if (tmask || rmask) walk<true, Write>(s, n, rows, TI, RI, tmask, rmask, in.nbpb, count, last, my_rec0, my_blk0, out, block, off_seg);
  else walk<false, Write>(s, n, rows, TI, RI, tmask, rmask, in.nbpb, count, last, my_rec0, my_blk0, out, block, off_seg);
  if (threadIdx.x == 0) {
    if (!Write) {
      cnt[slot] = count;
      last_block[slot] = last < 0 ? -1 : block_of_pos(rows[last].pos, in.nbpb);
    } else if (off) {
      if (count == 0) off_seg[0] = my_rec0;  // a chromosome without a used row owns one block, which is empty
      if (blockIdx.x == gridDim.x - 1) off[off_end] = rec_end;
    }
  }
}

template <class Out>
hipError_t launch(bool write, const DeviceInputs& in, int p0, int p1, int* cnt, int* last_block, const long long* rec0,
                  const int* blk0, const int* seg0, const Out out, int* block, long long* off, long long off_end,
                  long long rec_end, hipStream_t stream) {
  if (p1 <= p0 || in.C < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * in.C;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (write)
    hipLaunchKernelGGL((interval_walk_kernel<true, Out>), dim3((unsigned)grid), dim3(kTile), 0, stream, in, p0, cnt, last_block, rec0,
                       blk0, seg0, out, block, off, off_end, rec_end);
  else  // (the count pass writes no record: one instantiation serves both record forms)
    hipLaunchKernelGGL((interval_walk_kernel<false, IntervalOut>), dim3((unsigned)grid), dim3(kTile), 0, stream, in, p0, cnt, last_block,
                       rec0, blk0, seg0, IntervalOut{nullptr}, block, off, off_end, rec_end);
  return hipGetLastError();
}

}  // namespace

namespace colate_iw {

hipError_t count_launch(const DeviceInputs& in, int p0, int p1, int* cnt, int* last_block, hipStream_t stream) {
  return launch(false, in, p0, p1, cnt, last_block, nullptr, nullptr, nullptr, IntervalOut{nullptr}, nullptr, nullptr, 0, 0, stream);
}

hipError_t write_launch(const DeviceInputs& in, int p0, int p1, const long long* rec0, const int* blk0, const int* seg0,
                        IntervalRec* recs, int* block, long long* off, long long off_end, long long rec_end, hipStream_t stream) {
  return launch(true, in, p0, p1, nullptr, nullptr, rec0, blk0, seg0, IntervalOut{recs}, block, off, off_end, rec_end, stream);
}

hipError_t write_fill_launch(const DeviceInputs& in, int p0, int p1, const long long* rec0, const int* blk0, const int* seg0,
                             colate_drv::FillRec* recs, FillSide* side, long long* off, long long off_end, long long rec_end,
                             hipStream_t stream) {
  return launch(true, in, p0, p1, nullptr, nullptr, rec0, blk0, seg0, FillOut{recs, side}, nullptr, off, off_end, rec_end, stream);
}

}  // namespace colate_iw
