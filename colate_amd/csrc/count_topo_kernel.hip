// colate_amd/csrc/count_topo_kernel.hip -- `Colate --mode count_topo --samples` on the GPU (count_topo.h: the contract;
// count_topo.cpp: the host twin): the three kernels of the triple stage and the host code that drives them over the resident
// inputs of the pair walks (walk_resident.hpp), whose index arrays here are the S walk indices followed by the S cond indices.
//
//   * topo_planes_kernel: one lane per (array, searched row).  A wave holds the 64 rows of one plane word of one array: each
//     lane reads its 8-byte entry, forms `hit` (arrays 0 .. S - 1) or `qualifies` (arrays S .. 2 S - 1), and a ballot -- 64
//     bits on wave64 -- is the word, which lane 0 writes to planes[2 S][words] in HBM.  Every chromosome starts on a word;
//     lanes beyond the chromosome's end hold "no".
//   * topo_count_kernel: one workgroup (one wave) per (triple, chromosome): the lanes stride over the chromosome's words,
//     popc(hitT & hitR & qualC) is summed over the wave by shuffles and lane 0 writes cnt[p][c].
//   * topo_draw_kernel: one workgroup of four waves per (triple, chromosome).  Every wave goes through the chromosome tile by
//     tile, a tile being 64 words with one word per lane: popcount, an inclusive scan over the lanes by shuffles, and the
//     tile's total carried on -- so each wave knows every word's base rank without a barrier or LDS.  Wave w draws the tiles
//     w, w + 4, ...: word by word, lane = row, rank = base + popc(Q & lanes below); a lane whose bit is set reads u[2 rank],
//     u[2 rank + 1] and the target's and the reference's index entries (consecutive rows: coalesced), compares, and two ballots
//     are the `plus` and `minus` words, which the lane of that word keeps and the wave stores, one word per lane, at the end of
//     the tile.  Every output has one owner; a workgroup reads nothing another workgroup of the same launch writes.
// No atomics, no LDS, no barrier, no floating-point reduction, no compaction in these three.
//
// The age profile (colate_topo_profile) runs the same staging, planes and counts, and then
//   * topo_bins_kernel: one lane per searched row, once for all triples: the epochs in LDS, age_epoch as a binary search, the
//     row's epoch as 16 bits in HBM;
//   * topo_profile_kernel: the draw kernel's body (draw_tiles, shared by both) with another sink: where the draw kernel keeps a
//     word's two ballots, every lane with a set bit of Q reads its row's epoch and adds 1 to the workgroup's 3 x E histogram in
//     LDS -- integer adds, whose sum has no order --, and behind a barrier the workgroup writes its own 3 E words of partials.
//     No global atomics; the host sums the chromosomes' partials in long long.  No plane leaves the device.
//
// The profile per genome block (colate_topo_profile_blocks; count_topo.h: the blocks of this mode) runs the staging, planes and bins,
// with every block as a segment (chromosome, first row, end row) of the searched rows, and
//   * topo_block_count_kernel in place of the count kernel: one wave per (triple, block), the popcount of Q over the segment's
//     words, the first and the last one masked; from these the host forms every block's base rank behind the one wait;
//   * topo_block_profile_kernel: topo_profile_kernel per (triple, block).  draw_tiles takes a span -- the words gone through and
//     the rows kept of each: the whole chromosome for the two kernels above, whose code is what it was, or a segment's words with
//     the same masks --; a word cut by a block boundary is read by both neighbours and each keeps its own rows.  The same 3 x E
//     histogram and bins; the workgroup writes its own 3 E partials, zeros for a segment without a row.
//
// The expected counts per genome block (colate_topo_expected_blocks; count_topo.h: the expected counts) run the staging, planes, bins
// and segments, and nothing of the draws: no count kernel, no host wait, no rank and no stream of uniforms, since a row's addends
// depend on that row alone.
//   * topo_block_expected_kernel: one workgroup per (triple, block) over the segment's words; at every set bit of Q the two
//     fixed-point addends of expected_addends -- two 64-bit integer quotients, each a double first guess put right by its exact
//     integer remainder -- go into 64-bit LDS histograms, the row into a 32-bit one; the workgroup writes its 3 E integers as [E][3],
//     which the host copies into `counts` as they lie.  draw_tiles is not used and not touched.  No global atomics, no floating point
//     in the result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "count_topo.h"
#include "em_job.hpp"
#include "walk_resident.hpp"

using namespace colate;
using namespace colate_topo;
using colate_iw::DeviceInputs;

namespace {

__global__ __launch_bounds__(kPlaneTile) void topo_planes_kernel(DeviceInputs in, int S, unsigned long long* __restrict__ planes) {
  const int lane = threadIdx.x & 63;
  const long long gw = (long long)blockIdx.x * (kPlaneTile / 64) + (threadIdx.x >> 6);  // the word: alike in the whole wave
  if (gw >= in.words) return;
  const int a = blockIdx.y;  // the array: a walk index below S, a cond index from S on
  int c = 0;
  while (c + 1 < in.C && in.word_off[c + 1] <= gw) c++;  // (the chromosome of the word; empty chromosomes own no word)
  const long long r0 = in.row_off[c];
  const long long i = (gw - in.word_off[c]) * 64 + lane, n = in.row_off[c + 1] - r0;
  bool yes = false;
  if (i < n) {
    const Idx x = in.idx[(size_t)a * in.n + r0 + i];
    yes = a < S ? hits(x) : qualifies(x);
  }
  const unsigned long long w = __ballot(yes);
  if (lane == 0) planes[(size_t)a * in.words + gw] = w;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(64) void topo_count_kernel(DeviceInputs in, int S, const Triple* __restrict__ triples,
                                                        const unsigned long long* __restrict__ planes, int* __restrict__ cnt) {
  const int c = blockIdx.x % in.C, p = blockIdx.x / in.C;
  const int lane = threadIdx.x;
  const Triple t = triples[p];
  const long long w0 = in.word_off[c], W = in.word_off[c + 1] - w0;
  const unsigned long long* const hT = planes + (size_t)t.target * in.words + w0;
  const unsigned long long* const hR = planes + (size_t)t.reference * in.words + w0;
  const unsigned long long* const qC = planes + (size_t)(S + t.cond) * in.words + w0;
  int n = 0;
  for (long long k = lane; k < W; k += 64) n += __popcll(hT[k] & hR[k] & qC[k]);
  n = wave_sum(n);  // (a chromosome has fewer than 2^31 rows)
  if (lane == 0) cnt[(size_t)p * in.C + c] = n;
}

__device__ __forceinline__ unsigned long long wave_uniform(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// The words of a chromosome a workgroup goes through, and the rows it keeps of each.  All W words and every row:
struct WholeChromosome {
  __device__ __forceinline__ long long first() const { return 0; }
  __device__ __forceinline__ long long end(long long W) const { return W; }
  __device__ __forceinline__ unsigned long long keep(long long) const { return ~0ull; }
};
// ... or the rows [first, end) of a block (count_topo.h: Segment): the words they touch, the first and the last one masked.  A word
// cut by a block boundary belongs to both neighbours' ranges, and each keeps its own rows of it.  No row: no word.
struct SegmentWords {
  long long w_first, w_end;
  unsigned long long m_first, m_last;
  __device__ __forceinline__ explicit SegmentWords(const Segment& sg) {
    const bool any = sg.end > sg.first;
    w_first = any ? sg.first >> 6 : 0, w_end = any ? ((long long)sg.end + 63) >> 6 : 0;
    m_first = ~0ull << (sg.first & 63), m_last = (sg.end & 63) ? ~0ull >> (64 - (sg.end & 63)) : ~0ull;
  }
  __device__ __forceinline__ long long first() const { return w_first; }
  __device__ __forceinline__ long long end(long long) const { return w_end; }
  __device__ __forceinline__ unsigned long long keep(long long k) const {
    return (k == w_first ? m_first : ~0ull) & (k == w_end - 1 ? m_last : ~0ull);
  }
};

// The body of the draw kernel for the (triple, chromosome) of one workgroup, over what is done with a word: sink.begin() in front
// of a tile this wave draws, sink.word(w, kw, qw, plus, minus) at word w of the tile -- word kw of the chromosome, qw its Q,
// the two ballots of the signs -- where qw != 0, sink.end(k, inside) behind the tile for the lane's own word k.  No barrier and
// no LDS in here; the trip counts depend on the span's words alone.  span: the words gone through and the rows kept (above); carry:
// the rank of the span's first qualifying row.
template <class Sink, class Span = WholeChromosome>
__device__ __forceinline__ void draw_tiles(const DeviceInputs& in, int S, const Triple t, int c, long long carry,
                                           const unsigned long long* __restrict__ planes, const double* __restrict__ u, Sink& sink,
                                           const Span span = Span()) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long w0 = in.word_off[c], W = span.end(in.word_off[c + 1] - w0), r0 = in.row_off[c];
  const unsigned long long* const hT = planes + (size_t)t.target * in.words + w0;
  const unsigned long long* const hR = planes + (size_t)t.reference * in.words + w0;
  const unsigned long long* const qC = planes + (size_t)(S + t.cond) * in.words + w0;
  const Idx* const TI = in.idx + (size_t)t.target * in.n + r0;
  const Idx* const RI = in.idx + (size_t)t.reference * in.n + r0;
  for (long long tile0 = span.first(), tile = 0; tile0 < W; tile0 += kTileWords, tile++) {
    const long long k = tile0 + lane;
    const unsigned long long q = k < W ? hT[k] & hR[k] & qC[k] & span.keep(k) : 0ull;
    const int n = __popcll(q);
    int incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, 63, 64);
    if (tile % kDrawWaves == wave) {
      const int nw = (int)(W - tile0 < kTileWords ? W - tile0 : kTileWords);
      sink.begin();
      for (int w = 0; w < nw; w++) {
        const unsigned long long qw = wave_uniform(__shfl(q, w, 64));
        if (qw == 0) continue;  // (alike in the whole wave; the lane of this word keeps its zeros)
        const long long bw = carry + __shfl(incl - n, w, 64);
        int sign = 0;
        if ((qw >> lane) & 1) {
          const long long rank = bw + __popcll(qw & ((1ull << lane) - 1));
          const long long i = (tile0 + w) * 64 + lane;  // (a set bit of Q is a row of the chromosome)
          sign = draw_sign(TI[i], RI[i], u[2 * rank], u[2 * rank + 1]);
        }
        const unsigned long long a = __ballot(sign > 0), b = __ballot(sign < 0);
        sink.word(w, tile0 + w, qw, a, b);
      }
      sink.end(k, k < W);
    }
    carry += total;
  }
}

// the draw kernel's sink: the lane of a word keeps its two ballots and the wave stores them, one word per lane, behind the tile
struct StorePlanes {
  unsigned long long* pl;
  unsigned long long* mi;
  unsigned long long my_plus, my_minus;
  __device__ __forceinline__ void begin() { my_plus = 0, my_minus = 0; }
  __device__ __forceinline__ void word(int w, long long, unsigned long long, unsigned long long a, unsigned long long b) {
    if ((int)(threadIdx.x & 63) == w) my_plus = a, my_minus = b;
  }
  __device__ __forceinline__ void end(long long k, bool inside) {
    if (inside) pl[k] = my_plus, mi[k] = my_minus;
  }
};

__global__ __launch_bounds__(kDrawWaves * 64) void topo_draw_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                                    const unsigned long long* __restrict__ planes,
                                                                    const long long* __restrict__ base, const double* __restrict__ u,
                                                                    unsigned long long* __restrict__ plus, unsigned long long* __restrict__ minus) {
  const int c = blockIdx.x % in.C, j = blockIdx.x / in.C;  // (triple p0 + j, chromosome c)
  const long long w0 = in.word_off[c];
  StorePlanes sink{plus + (size_t)j * in.words + w0, minus + (size_t)j * in.words + w0, 0, 0};
  // base: the rank of the chromosome's first qualifying row
  draw_tiles(in, S, triples[p0 + j], c, base[(size_t)(p0 + j) * in.C + c], planes, u, sink);
}

// bin[i] = age_epoch of searched row i, the chromosomes back to back: one lane per row.  The workgroup loads the epochs -- 8 KB at
// most -- into LDS behind one barrier, which every thread reaches; the search takes 10 steps at most.
__global__ __launch_bounds__(kPlaneTile) void topo_bins_kernel(const Row* __restrict__ rows, long long n, int E, const double* __restrict__ epochs,
                                                               unsigned short* __restrict__ bin) {
  __shared__ double ep[kMaxProfileEpochs];
  for (int e = threadIdx.x; e < E; e += kPlaneTile) ep[e] = epochs[e];
  __syncthreads();
  const long long i = (long long)blockIdx.x * kPlaneTile + threadIdx.x;
  if (i < n) bin[i] = (unsigned short)age_epoch(rows[i].age_begin, rows[i].age_end, ep, E);
}

// the profile kernel's sink: every lane with a set bit of Q counts its row in the row's epoch -- qualifying, and plus or minus by
// its sign.  Integer adds in LDS: their sum has no order.
struct BinRows {
  const unsigned short* bin;  // of the chromosome's first row
  unsigned* hist;             // [3][E]: plus, minus, qualifying
  int E;
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void word(int, long long kw, unsigned long long qw, unsigned long long a, unsigned long long b) {
    const int lane = threadIdx.x & 63;
    if ((qw >> lane) & 1) {
      const int e = bin[kw * 64 + lane];  // (a set bit of Q is a row of the chromosome; bins_launch wrote 0 .. E - 1)
      atomicAdd(&hist[2 * E + e], 1u);
      if ((a >> lane) & 1) atomicAdd(&hist[e], 1u);
      else if ((b >> lane) & 1) atomicAdd(&hist[E + e], 1u);
    }
  }
  __device__ __forceinline__ void end(long long, bool) {}
};

// One workgroup of kDrawWaves waves per (triple, chromosome): the histogram zeroed behind a barrier, the draws, a second barrier,
// and the workgroup's own 3 E words of `part`.  Both barriers are reached by every wave.
__global__ __launch_bounds__(kDrawWaves * 64) void topo_profile_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                                       const unsigned long long* __restrict__ planes,
                                                                       const long long* __restrict__ base, const double* __restrict__ u,
                                                                       const unsigned short* __restrict__ bin, int E, unsigned* __restrict__ part) {
  __shared__ unsigned hist[3 * kMaxProfileEpochs];
  const int c = blockIdx.x % in.C, j = blockIdx.x / in.C;  // (triple p0 + j, chromosome c)
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) hist[i] = 0;
  __syncthreads();
  BinRows sink{bin + in.row_off[c], hist, E};
  draw_tiles(in, S, triples[p0 + j], c, base[(size_t)(p0 + j) * in.C + c], planes, u, sink);
  __syncthreads();
  unsigned* const mine = part + (size_t)blockIdx.x * 3 * (size_t)E;
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) mine[i] = hist[i];
}

// One wave per (triple, block): popc(Q) over the segment's words, the first and the last one masked; lane 0 writes cnt[p][b].
__global__ __launch_bounds__(64) void topo_block_count_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                              const unsigned long long* __restrict__ planes, int nb,
                                                              const Segment* __restrict__ seg, int* __restrict__ cnt) {
  const int b = blockIdx.x % nb, j = blockIdx.x / nb;  // (triple p0 + j, block b)
  const int lane = threadIdx.x;
  const Triple t = triples[p0 + j];
  const Segment sg = seg[b];
  const SegmentWords span(sg);
  const long long w0 = in.word_off[sg.c];
  const unsigned long long* const hT = planes + (size_t)t.target * in.words + w0;
  const unsigned long long* const hR = planes + (size_t)t.reference * in.words + w0;
  const unsigned long long* const qC = planes + (size_t)(S + t.cond) * in.words + w0;
  int n = 0;
  for (long long k = span.w_first + lane; k < span.w_end; k += 64) n += __popcll(hT[k] & hR[k] & qC[k] & span.keep(k));
  n = wave_sum(n);  // (a chromosome has fewer than 2^31 rows)
  if (lane == 0) cnt[(size_t)(p0 + j) * nb + b] = n;
}

// One workgroup of kDrawWaves waves per (triple, block): topo_profile_kernel over the words of the block's segment.  base: the rank
// of the block's first qualifying row; an empty segment goes through no word and writes zeros.  Both barriers are reached by every
// wave.
__global__ __launch_bounds__(kDrawWaves * 64) void topo_block_profile_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                                             const unsigned long long* __restrict__ planes, int nb,
                                                                             const Segment* __restrict__ seg, const long long* __restrict__ base,
                                                                             const double* __restrict__ u, const unsigned short* __restrict__ bin,
                                                                             int E, unsigned* __restrict__ part) {
  __shared__ unsigned hist[3 * kMaxProfileEpochs];
  const int b = blockIdx.x % nb, j = blockIdx.x / nb;  // (triple p0 + j, block b)
  const Segment sg = seg[b];
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) hist[i] = 0;
  __syncthreads();
  BinRows sink{bin + in.row_off[sg.c], hist, E};
  draw_tiles(in, S, triples[p0 + j], sg.c, base[(size_t)(p0 + j) * nb + b], planes, u, sink, SegmentWords(sg));
  __syncthreads();
  unsigned* const mine = part + (size_t)blockIdx.x * 3 * (size_t)E;
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) mine[i] = hist[i];
}

// One workgroup of kDrawWaves waves per (triple, block): the expected counts of the block (count_topo.h: expected_addends).  Wave w
// takes the tiles w, w + kDrawWaves, ... of the segment's words, a tile being 64 words with one word per lane, masked as SegmentWords
// masks them; a ballot names the words of the tile with a set bit of Q, and at each of those, lane = row, a lane whose bit is set reads
// the target's and the reference's index entries and its row's epoch, forms the two addends and adds them -- and 1 for the row -- to
// the workgroup's histograms in LDS: [2][E] 64-bit sums, [E] 32-bit rows (a segment has fewer than 2^31 rows), 20 E bytes.  A zero
// addend is not added: where T and R are fixed one of the two always is.  Integer adds, whose sum has no order; no rank, no uniform,
// nothing carried from tile to tile.  Both barriers are reached by every wave, whatever its trip count; behind the second the
// workgroup writes its own 3 E integers as [E][3], the layout of `counts`: zeros where the segment holds no row.
__global__ __launch_bounds__(kDrawWaves * 64) void topo_block_expected_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                                              const unsigned long long* __restrict__ planes, int nb,
                                                                              const Segment* __restrict__ seg, const unsigned short* __restrict__ bin,
                                                                              int E, long long* __restrict__ part) {
  __shared__ unsigned long long sums[2 * kMaxProfileEpochs];
  __shared__ unsigned rows_in[kMaxProfileEpochs];
  const int b = blockIdx.x % nb, j = blockIdx.x / nb;  // (triple p0 + j, block b)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Triple t = triples[p0 + j];
  const Segment sg = seg[b];
  const SegmentWords span(sg);
  for (int i = threadIdx.x; i < 2 * E; i += kDrawWaves * 64) sums[i] = 0;
  for (int i = threadIdx.x; i < E; i += kDrawWaves * 64) rows_in[i] = 0;
  __syncthreads();
  const long long w0 = in.word_off[sg.c], r0 = in.row_off[sg.c];
  const unsigned long long* const hT = planes + (size_t)t.target * in.words + w0;
  const unsigned long long* const hR = planes + (size_t)t.reference * in.words + w0;
  const unsigned long long* const qC = planes + (size_t)(S + t.cond) * in.words + w0;
  const Idx* const TI = in.idx + (size_t)t.target * in.n + r0;
  const Idx* const RI = in.idx + (size_t)t.reference * in.n + r0;
  const unsigned short* const epoch_of = bin + r0;
  for (long long tile0 = span.w_first + (long long)wave * kTileWords; tile0 < span.w_end; tile0 += kDrawWaves * kTileWords) {
    const long long k = tile0 + lane;
    const unsigned long long q = k < span.w_end ? hT[k] & hR[k] & qC[k] & span.keep(k) : 0ull;
    for (unsigned long long left = __ballot(q != 0); left; left &= left - 1) {  // (alike in the whole wave)
      const int w = __builtin_ctzll(left);
      const unsigned long long qw = wave_uniform(__shfl(q, w, 64));
      if ((qw >> lane) & 1) {
        const long long i = (tile0 + w) * 64 + lane;  // (a set bit of Q is a row of the chromosome, and of the segment by the mask)
        const Addends x = expected_addends(TI[i], RI[i]);
        const int e = epoch_of[i];  // (bins_launch wrote 0 .. E - 1)
        if (x.plus) atomicAdd(&sums[e], x.plus);
        if (x.minus) atomicAdd(&sums[E + e], x.minus);
        atomicAdd(&rows_in[e], 1u);
      }
    }
  }
  __syncthreads();
  long long* const mine = part + (size_t)blockIdx.x * 3 * (size_t)E;
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) {
    const int e = i / 3, which = i - 3 * e;
    mine[i] = which < 2 ? (long long)sums[which * E + e] : (long long)rows_in[e];
  }
}

thread_local int g_chunks = 0, g_profile_chunks = 0, g_blocks_chunks = 0, g_expected_chunks = 0;
thread_local double g_kernel_s = 0.0, g_profile_kernel_s = 0.0, g_blocks_kernel_s = 0.0, g_expected_kernel_s = 0.0;

// bytes of what a chunk of triples leaves on the device -- the two output planes of colate_topo_samples, the partial histograms
// of colate_topo_profile -- (COLATE_TOPO_BUDGET: bytes, for the tests)
long long output_budget() {
  if (const char* e = std::getenv("COLATE_TOPO_BUDGET")) return std::max(1LL, std::atoll(e));
  return 256LL << 20;
}

// What the device calls stage on the workspace's stream in front of their chunks of triples: the inputs resident, the planes,
// the counts with the one host wait for them, every (triple, chromosome)'s first rank and the uniforms the longest triple needs.
// With G and count given, the groups of a triple are not its C chromosomes: count(d_cnt) launches what fills cnt[P][G], the
// groups in the genome's order (colate_topo_profile_blocks: the blocks).
struct Front {
  colate_iw::Resident res;
  DeviceBuffers buf;
  std::vector<const Idx*> both;  // the walk indices, then the cond indices
  std::vector<int> cnt;
  std::vector<long long> base, n;  // [P][G], [P]: the qualifying rows
  unsigned long long* d_planes = nullptr;
  Triple* d_triples = nullptr;
  long long* d_base = nullptr;
  double* d_u = nullptr;
  int stage(const View& v, long long words, hipStream_t stream, colate_iw::KernelTimer& timer) {
    return stage(v, words, stream, timer, v.C, [&](int* d_cnt) {
      if (hipError_t e = count_launch(res.in, v.S, v.P, d_triples, d_planes, d_cnt, stream)) return hip_fail(e, "topo count kernel launch");
      return (int)COLATE_OK;
    });
  }
  template <class Count>
  int stage(const View& v, long long words, hipStream_t stream, colate_iw::KernelTimer& timer, int G, Count&& count) {
    const size_t PC = (size_t)v.P * (size_t)G;
    cnt.resize(PC), base.resize(PC), n.assign((size_t)v.P, 0), both.resize((size_t)2 * v.S * v.C);
    std::copy_n(v.idx, (size_t)v.S * v.C, both.begin());
    std::copy_n(v.cidx, (size_t)v.S * v.C, both.begin() + (size_t)v.S * v.C);
    colate_iw::View iv;
    iv.C = v.C, iv.row_off = v.row_off, iv.rows = v.rows, iv.S = 2 * v.S, iv.idx = both.data(), iv.M = 0, iv.P = 0, iv.pairs = nullptr, iv.nbpb = 1;
    if (int rc = res.upload(iv, stream)) return rc;
    int* d_cnt = nullptr;
    HIP_TRY(buf.device(d_planes, (size_t)2 * v.S * (size_t)words)); HIP_TRY(buf.device(d_triples, (size_t)v.P));
    HIP_TRY(buf.device(d_cnt, PC)); HIP_TRY(buf.device(d_base, PC));
    HIP_TRY(colate_iw::h2d(stream, d_triples, v.triples, sizeof(Triple) * (size_t)v.P));
    HIP_TRY(timer.mark());
    if (hipError_t e = planes_launch(res.in, v.S, d_planes, stream)) return hip_fail(e, "topo planes kernel launch");
    if (int rc = count(d_cnt)) return rc;
    HIP_TRY(timer.mark());
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * PC, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the one wait for the counts
    long long most = 0;
    for (int p = 0; p < v.P; p++) {
      for (int c = 0; c < G; c++) base[(size_t)p * G + c] = n[(size_t)p], n[(size_t)p] += cnt[(size_t)p * G + c];
      most = std::max(most, n[(size_t)p]);
    }
    if (int rc = check_stream(v, n.data())) return rc;
    // every triple starts from the run's seed: one stream for all, as long as the longest needs
    HIP_TRY(buf.device(d_u, (size_t)(2 * most)));
    HIP_TRY(colate_iw::h2d(stream, d_u, v.uniforms, sizeof(double) * (size_t)(2 * most)));
    HIP_TRY(colate_iw::h2d(stream, d_base, base.data(), sizeof(long long) * PC));
    return COLATE_OK;
  }
};

int check_grids_of(const View& v) {
  if (2LL * v.S > 65535) return fail(COLATE_ELIMIT, "S=%d above the grid of the plane kernel (32767)", v.S);
  if ((long long)v.P * v.C > 0x7fffffffLL) return fail(COLATE_ELIMIT, "P x C = %lld above the grid of the count kernel", (long long)v.P * v.C);
  return COLATE_OK;
}

}  // namespace

namespace colate_topo {

hipError_t planes_launch(const DeviceInputs& in, int S, unsigned long long* planes, hipStream_t stream) {
  if (in.words < 1 || in.S < 1) return hipSuccess;
  const long long blocks = (in.words + kPlaneTile / 64 - 1) / (kPlaneTile / 64);
  if (blocks > 0x7fffffffLL || in.S > 65535 || in.S != 2 * S) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_planes_kernel, dim3((unsigned)blocks, (unsigned)in.S), dim3(kPlaneTile), 0, stream, in, S, planes);
  return hipGetLastError();
}

hipError_t count_launch(const DeviceInputs& in, int S, int P, const Triple* triples, const unsigned long long* planes, int* cnt,
                        hipStream_t stream) {
  if (P < 1 || in.C < 1) return hipSuccess;
  const long long grid = (long long)P * in.C;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_count_kernel, dim3((unsigned)grid), dim3(64), 0, stream, in, S, triples, planes, cnt);
  return hipGetLastError();
}

hipError_t draw_launch(const DeviceInputs& in, int S, int p0, int p1, const Triple* triples, const unsigned long long* planes,
                       const long long* base, const double* u, unsigned long long* plus, unsigned long long* minus, hipStream_t stream) {
  if (p1 <= p0 || in.C < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * in.C;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_draw_kernel, dim3((unsigned)grid), dim3(kDrawWaves * 64), 0, stream, in, S, p0, triples, planes, base, u, plus, minus);
  return hipGetLastError();
}

hipError_t bins_launch(const DeviceInputs& in, int E, const double* epochs, unsigned short* bin, hipStream_t stream) {
  if (in.n < 1) return hipSuccess;
  const long long blocks = (in.n + kPlaneTile - 1) / kPlaneTile;
  if (blocks > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_bins_kernel, dim3((unsigned)blocks), dim3(kPlaneTile), 0, stream, in.rows, in.n, E, epochs, bin);
  return hipGetLastError();
}

hipError_t profile_launch(const DeviceInputs& in, int S, int p0, int p1, const Triple* triples, const unsigned long long* planes,
                          const long long* base, const double* u, const unsigned short* bin, int E, unsigned* part, hipStream_t stream) {
  if (p1 <= p0 || in.C < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * in.C;
  if (grid > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_profile_kernel, dim3((unsigned)grid), dim3(kDrawWaves * 64), 0, stream, in, S, p0, triples, planes, base, u, bin, E, part);
  return hipGetLastError();
}

hipError_t block_count_launch(const DeviceInputs& in, int S, int p0, int p1, const Triple* triples, const unsigned long long* planes, int nb,
                              const Segment* seg, int* cnt, hipStream_t stream) {
  if (p1 <= p0 || nb < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * nb;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_block_count_kernel, dim3((unsigned)grid), dim3(64), 0, stream, in, S, p0, triples, planes, nb, seg, cnt);
  return hipGetLastError();
}

hipError_t block_profile_launch(const DeviceInputs& in, int S, int p0, int p1, const Triple* triples, const unsigned long long* planes, int nb,
                                const Segment* seg, const long long* base, const double* u, const unsigned short* bin, int E, unsigned* part,
                                hipStream_t stream) {
  if (p1 <= p0 || nb < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * nb;
  if (grid > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_block_profile_kernel, dim3((unsigned)grid), dim3(kDrawWaves * 64), 0, stream, in, S, p0, triples, planes, nb, seg, base, u,
                     bin, E, part);
  return hipGetLastError();
}

hipError_t block_expected_launch(const DeviceInputs& in, int S, int p0, int p1, const Triple* triples, const unsigned long long* planes, int nb,
                                 const Segment* seg, const unsigned short* bin, int E, long long* part, hipStream_t stream) {
  if (p1 <= p0 || nb < 1) return hipSuccess;
  const long long grid = (long long)(p1 - p0) * nb;
  if (grid > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_block_expected_kernel, dim3((unsigned)grid), dim3(kDrawWaves * 64), 0, stream, in, S, p0, triples, planes, nb, seg, bin, E,
                     part);
  return hipGetLastError();
}

int topo_view_device(const View& v, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws) {
  if (int rc = check_outputs(cap, word_off, plus, minus, draws)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = check_grids_of(v)) return rc;
  std::vector<long long> woff((size_t)v.C + 1);
  const long long words = colate_iw::mask_words(v.C, v.row_off, woff.data());
  if (int rc = check_capacity(v.P, words, cap)) return rc;
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_topo_samples: H2D + planes + counts; the uniforms; per chunk of triples the draws + D2H");
  g_chunks = 0, g_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  colate_iw::KernelTimer timer(stream);
  Front f;
  const colate_iw::StreamSync sync_at_exit{stream};
  // triples per chunk: the two output planes of a chunk within the budget, and the grid within 2^31 workgroups
  const long long per_triple = std::max(1LL, 2 * words * (long long)sizeof(unsigned long long));
  const long long chunk = std::max(1LL, std::min<long long>({(long long)v.P, output_budget() / per_triple, 0x7fffffffLL / v.C}));
  unsigned long long *d_plus = nullptr, *d_minus = nullptr;
  HIP_TRY(f.buf.device(d_plus, (size_t)(chunk * words))); HIP_TRY(f.buf.device(d_minus, (size_t)(chunk * words)));
  if (int rc = f.stage(v, words, stream, timer)) return rc;
  for (long long p0 = 0; p0 < v.P; p0 += chunk) {  // (a chunk's planes are copied out before the next launch overwrites them: one stream)
    const long long p1 = std::min<long long>(v.P, p0 + chunk);
    HIP_TRY(timer.mark());
    if (hipError_t e = draw_launch(f.res.in, v.S, (int)p0, (int)p1, f.d_triples, f.d_planes, f.d_base, f.d_u, d_plus, d_minus, stream))
      return hip_fail(e, "topo draw kernel launch");
    HIP_TRY(timer.mark());
    const size_t bytes = sizeof(unsigned long long) * (size_t)((p1 - p0) * words);
    if (bytes) {
      HIP_TRY(hipMemcpyAsync(plus + p0 * words, d_plus, bytes, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipMemcpyAsync(minus + p0 * words, d_minus, bytes, hipMemcpyDeviceToHost, stream));
    }
    g_chunks++;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  g_kernel_s = timer.seconds();
  std::memcpy(draws, f.n.data(), sizeof(long long) * (size_t)v.P);
  std::memcpy(word_off, woff.data(), sizeof(long long) * woff.size());
  return COLATE_OK;
}

int topo_profile_device(const View& v, int E, const double* epochs, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = check_grids_of(v)) return rc;
  if ((v.row_off[v.C] + kPlaneTile - 1) / kPlaneTile > 0x7fffffffLL)
    return fail(COLATE_ELIMIT, "%lld rows above the grid of the bins kernel", v.row_off[v.C]);
  std::vector<long long> woff((size_t)v.C + 1);
  const long long words = colate_iw::mask_words(v.C, v.row_off, woff.data());
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_topo_profile: H2D + planes + counts + bins; the uniforms; per chunk of triples the binned draws + D2H");
  g_profile_chunks = 0, g_profile_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  colate_iw::KernelTimer timer(stream);
  Front f;
  // triples per chunk: the partial histograms of a chunk -- 12 E bytes per (triple, chromosome) -- within the budget, and the grid
  // within 2^31 workgroups
  const size_t per_block = 3 * (size_t)E;
  const long long per_triple = (long long)(per_block * sizeof(unsigned)) * v.C;
  const long long chunk = std::max(1LL, std::min<long long>({(long long)v.P, output_budget() / per_triple, 0x7fffffffLL / v.C}));
  std::vector<unsigned> part((size_t)chunk * v.C * per_block);
  const colate_iw::StreamSync sync_at_exit{stream};
  unsigned short* d_bin = nullptr;
  double* d_epochs = nullptr;
  unsigned* d_part = nullptr;
  HIP_TRY(f.buf.device(d_bin, (size_t)v.row_off[v.C])); HIP_TRY(f.buf.device(d_epochs, (size_t)E)); HIP_TRY(f.buf.device(d_part, part.size()));
  if (int rc = f.stage(v, words, stream, timer)) return rc;
  HIP_TRY(colate_iw::h2d(stream, d_epochs, epochs, sizeof(double) * (size_t)E));
  HIP_TRY(timer.mark());
  if (hipError_t e = bins_launch(f.res.in, E, d_epochs, d_bin, stream)) return hip_fail(e, "topo bins kernel launch");  // once, for every triple
  HIP_TRY(timer.mark());
  std::memset(counts, 0, sizeof(long long) * (size_t)v.P * per_block);
  for (long long p0 = 0; p0 < v.P; p0 += chunk) {
    const long long p1 = std::min<long long>(v.P, p0 + chunk);
    HIP_TRY(timer.mark());
    if (hipError_t e = profile_launch(f.res.in, v.S, (int)p0, (int)p1, f.d_triples, f.d_planes, f.d_base, f.d_u, d_bin, E, d_part, stream))
      return hip_fail(e, "topo profile kernel launch");
    HIP_TRY(timer.mark());
    HIP_TRY(hipMemcpyAsync(part.data(), d_part, sizeof(unsigned) * (size_t)(p1 - p0) * v.C * per_block, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // (the one wait at the end where one chunk holds every triple)
    for (long long p = p0; p < p1; p++)  // the chromosomes' partials, summed in long long
      for (int c = 0; c < v.C; c++) {
        const unsigned* const h = part.data() + ((size_t)(p - p0) * v.C + c) * per_block;
        long long* const out = counts + (size_t)p * per_block;
        for (int e = 0; e < E; e++) out[3 * e] += h[e], out[3 * e + 1] += h[E + e], out[3 * e + 2] += h[2 * E + e];
      }
    g_profile_chunks++;
  }
  g_profile_kernel_s = timer.seconds();
  std::memcpy(draws, f.n.data(), sizeof(long long) * (size_t)v.P);
  return COLATE_OK;
}

int topo_profile_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  std::vector<int> blk_off;
  if (int rc = check_blocks(v, E, nbpb, nb, blk_off)) return rc;
  if (int rc = check_grids_of(v)) return rc;
  if ((v.row_off[v.C] + kPlaneTile - 1) / kPlaneTile > 0x7fffffffLL)
    return fail(COLATE_ELIMIT, "%lld rows above the grid of the bins kernel", v.row_off[v.C]);
  std::vector<long long> woff((size_t)v.C + 1);
  const long long words = colate_iw::mask_words(v.C, v.row_off, woff.data());
  std::vector<Segment> seg((size_t)nb);
  block_segments(v, nbpb, blk_off.data(), seg.data());
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_topo_profile_blocks: H2D + planes + block counts + bins; the uniforms; per chunk of triples the binned draws of every block + D2H");
  g_blocks_chunks = 0, g_blocks_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  colate_iw::KernelTimer timer(stream);
  Front f;
  // triples per chunk: the partial histograms of a chunk -- 12 E bytes per (triple, block) -- within the budget, and the grid within
  // 2^31 workgroups; one triple where its partials alone are above the budget
  const size_t per_block = 3 * (size_t)E;
  const long long per_triple = (long long)(per_block * sizeof(unsigned)) * nb;
  const long long grid_most = 0x7fffffffLL / nb;
  const long long chunk = std::max(1LL, std::min<long long>({(long long)v.P, output_budget() / per_triple, grid_most}));
  std::vector<unsigned> part((size_t)chunk * (size_t)nb * per_block);
  const colate_iw::StreamSync sync_at_exit{stream};
  unsigned short* d_bin = nullptr;
  double* d_epochs = nullptr;
  unsigned* d_part = nullptr;
  Segment* d_seg = nullptr;
  HIP_TRY(f.buf.device(d_bin, (size_t)v.row_off[v.C])); HIP_TRY(f.buf.device(d_epochs, (size_t)E)); HIP_TRY(f.buf.device(d_part, part.size()));
  HIP_TRY(f.buf.device(d_seg, (size_t)nb));
  HIP_TRY(colate_iw::h2d(stream, d_seg, seg.data(), sizeof(Segment) * (size_t)nb));
  // the counts per (triple, block) take the place of those per (triple, chromosome): a block's base is the sum of the blocks in front
  const int staged = f.stage(v, words, stream, timer, nb, [&](int* d_cnt) {
    for (long long p0 = 0; p0 < v.P; p0 += grid_most)
      if (hipError_t e = block_count_launch(f.res.in, v.S, (int)p0, (int)std::min<long long>(v.P, p0 + grid_most), f.d_triples, f.d_planes, nb, d_seg,
                                            d_cnt, stream))
        return hip_fail(e, "topo block count kernel launch");
    return (int)COLATE_OK;
  });
  if (staged) return staged;
  HIP_TRY(colate_iw::h2d(stream, d_epochs, epochs, sizeof(double) * (size_t)E));
  HIP_TRY(timer.mark());
  if (hipError_t e = bins_launch(f.res.in, E, d_epochs, d_bin, stream)) return hip_fail(e, "topo bins kernel launch");  // once, for every triple
  HIP_TRY(timer.mark());
  for (long long p0 = 0; p0 < v.P; p0 += chunk) {
    const long long p1 = std::min<long long>(v.P, p0 + chunk);
    HIP_TRY(timer.mark());
    if (hipError_t e = block_profile_launch(f.res.in, v.S, (int)p0, (int)p1, f.d_triples, f.d_planes, nb, d_seg, f.d_base, f.d_u, d_bin, E, d_part,
                                            stream))
      return hip_fail(e, "topo block profile kernel launch");
    HIP_TRY(timer.mark());
    HIP_TRY(hipMemcpyAsync(part.data(), d_part, sizeof(unsigned) * (size_t)(p1 - p0) * (size_t)nb * per_block, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // (the one wait at the end where one chunk holds every triple)
    for (size_t k = 0; k < (size_t)(p1 - p0) * (size_t)nb; k++) {  // every (triple, block) owns its partials: [3][E] into [E][3]
      const unsigned* const h = part.data() + k * per_block;
      long long* const out = counts + ((size_t)p0 * (size_t)nb + k) * per_block;
      for (int e = 0; e < E; e++) out[3 * e] = h[e], out[3 * e + 1] = h[E + e], out[3 * e + 2] = h[2 * E + e];
    }
    g_blocks_chunks++;
  }
  g_blocks_kernel_s = timer.seconds();
  std::memcpy(draws, f.n.data(), sizeof(long long) * (size_t)v.P);
  return COLATE_OK;
}

int topo_expected_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts) {
  std::vector<int> blk_off;
  if (int rc = check_expected(v, E, epochs, nbpb, nb, counts, blk_off)) return rc;
  if (int rc = check_grids_of(v)) return rc;
  std::vector<long long> woff((size_t)v.C + 1);
  const long long words = colate_iw::mask_words(v.C, v.row_off, woff.data());
  std::vector<Segment> seg((size_t)nb);
  block_segments(v, nbpb, blk_off.data(), seg.data());
  if (int rc = ensure_device()) return rc;
  ProfRange range("colate_topo_expected_blocks: H2D + planes + bins; per chunk of triples the expected counts of every block + D2H");
  g_expected_chunks = 0, g_expected_kernel_s = 0.0;
  if (int rc = thread_workspace().reserve(256, 256)) return rc;  // (the workspace's stream: no second one)
  hipStream_t stream = thread_workspace().stream;
  colate_iw::KernelTimer timer(stream);
  colate_iw::Resident res;
  DeviceBuffers buf;
  // triples per chunk: the partials of a chunk -- 24 E bytes per (triple, block) -- within the budget, and the grid within 2^31
  // workgroups; one triple where its partials alone are above the budget
  const size_t per_block = 3 * (size_t)E;
  const long long per_triple = (long long)(per_block * sizeof(long long)) * nb;
  const long long chunk = std::max(1LL, std::min<long long>({(long long)v.P, output_budget() / per_triple, 0x7fffffffLL / nb}));
  const colate_iw::StreamSync sync_at_exit{stream};
  std::vector<const Idx*> both((size_t)2 * v.S * v.C);  // the walk indices, then the cond indices
  std::copy_n(v.idx, (size_t)v.S * v.C, both.begin());
  std::copy_n(v.cidx, (size_t)v.S * v.C, both.begin() + (size_t)v.S * v.C);
  colate_iw::View iv;
  iv.C = v.C, iv.row_off = v.row_off, iv.rows = v.rows, iv.S = 2 * v.S, iv.idx = both.data(), iv.M = 0, iv.P = 0, iv.pairs = nullptr, iv.nbpb = 1;
  if (int rc = res.upload(iv, stream)) return rc;
  unsigned long long* d_planes = nullptr;
  Triple* d_triples = nullptr;
  unsigned short* d_bin = nullptr;
  double* d_epochs = nullptr;
  long long* d_part = nullptr;
  Segment* d_seg = nullptr;
  HIP_TRY(buf.device(d_planes, (size_t)2 * v.S * (size_t)words)); HIP_TRY(buf.device(d_triples, (size_t)v.P));
  HIP_TRY(buf.device(d_bin, (size_t)v.row_off[v.C])); HIP_TRY(buf.device(d_epochs, (size_t)E));
  HIP_TRY(buf.device(d_part, (size_t)chunk * (size_t)nb * per_block)); HIP_TRY(buf.device(d_seg, (size_t)nb));
  HIP_TRY(colate_iw::h2d(stream, d_triples, v.triples, sizeof(Triple) * (size_t)v.P));
  HIP_TRY(colate_iw::h2d(stream, d_seg, seg.data(), sizeof(Segment) * (size_t)nb));
  HIP_TRY(colate_iw::h2d(stream, d_epochs, epochs, sizeof(double) * (size_t)E));
  HIP_TRY(timer.mark());
  if (hipError_t e = planes_launch(res.in, v.S, d_planes, stream)) return hip_fail(e, "topo planes kernel launch");
  if (hipError_t e = bins_launch(res.in, E, d_epochs, d_bin, stream)) return hip_fail(e, "topo bins kernel launch");  // once, for every triple
  HIP_TRY(timer.mark());
  for (long long p0 = 0; p0 < v.P; p0 += chunk) {  // (a chunk's partials are copied out before the next launch overwrites them: one stream)
    const long long p1 = std::min<long long>(v.P, p0 + chunk);
    HIP_TRY(timer.mark());
    if (hipError_t e = block_expected_launch(res.in, v.S, (int)p0, (int)p1, d_triples, d_planes, nb, d_seg, d_bin, E, d_part, stream))
      return hip_fail(e, "topo block expected kernel launch");
    HIP_TRY(timer.mark());
    // every (triple, block) owns its partials, written as [E][3]: they are `counts` as they lie
    HIP_TRY(hipMemcpyAsync(counts + (size_t)p0 * (size_t)nb * per_block, d_part, sizeof(long long) * (size_t)(p1 - p0) * (size_t)nb * per_block,
                           hipMemcpyDeviceToHost, stream));
    g_expected_chunks++;
  }
  HIP_TRY(hipStreamSynchronize(stream));  // the one wait of the call
  g_expected_kernel_s = timer.seconds();
  return COLATE_OK;
}

}  // namespace colate_topo

extern "C" {
int colate_topo_expected_blocks_chunks(void) { return g_expected_chunks; }
double colate_topo_expected_blocks_kernel_seconds(void) { return g_expected_kernel_s; }
int colate_topo_profile_blocks_chunks(void) { return g_blocks_chunks; }
double colate_topo_profile_blocks_kernel_seconds(void) { return g_blocks_kernel_s; }
int colate_topo_samples_chunks(void) { return g_chunks; }
double colate_topo_samples_kernel_seconds(void) { return g_kernel_s; }
int colate_topo_profile_chunks(void) { return g_profile_chunks; }
double colate_topo_profile_kernel_seconds(void) { return g_profile_kernel_s; }
}
