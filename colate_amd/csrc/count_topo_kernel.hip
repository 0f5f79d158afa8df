// colate_amd/csrc/count_topo_kernel.hip -- `Colate --mode count_topo --samples` on the GPU (count_topo.h: the contract;
// count_topo.cpp: the host twin): the three kernels of the triple stage and the host code that drives them over the resident
// inputs of the pair walks (walk_resident.hpp), whose index arrays here are the S walk indices followed by the S cond indices.
//
//   * topo_planes_kernel: one lane per (array, searched row).  A wave holds the 64 rows of one plane word of one array: each
//     lane reads its 8-byte entry, forms `hit` (arrays 0 .. S - 1) or `qualifies` (arrays S .. 2 S - 1), and a ballot -- 64
//     bits on wave64 -- is the word, which lane 0 writes to planes[2 S][words] in HBM.  Every chromosome starts on a word;
//     lanes beyond the chromosome's end hold "no".
//   * topo_count_kernel<Chromosomes>: one workgroup (one wave) per (triple, chromosome): the lanes stride over the chromosome's
//     words, popc(hitT & hitR & qualC) is summed over the wave by shuffles and lane 0 writes cnt[p][c].
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
//   * topo_profile_kernel<Chromosomes>: the draw kernel's body (draw_tiles, shared by both) with another sink: where the draw kernel
//     keeps a word's two ballots, every lane with a set bit of Q reads its row's epoch and adds 1 to the workgroup's 3 x E histogram
//     in LDS -- integer adds, whose sum has no order --, and behind a barrier the workgroup writes its own 3 E words of partials.
//     No global atomics; the host sums the chromosomes' partials in long long.  No plane leaves the device.
//
// The count and the profile kernel are written once, over the GROUPS of a triple (Chromosomes, Blocks): a group is a chromosome, whole,
// or a block of this mode (count_topo.h) as a segment (chromosome, first row, end row) of the searched rows.  The profile per genome
// block (colate_topo_profile_blocks) runs the staging, planes and bins, and
//   * topo_count_kernel<Blocks> in place of the count over chromosomes: one wave per (triple, block), the popcount of Q over the
//     segment's words, the first and the last one masked; from these the host forms every block's base rank behind the one wait;
//   * topo_profile_kernel<Blocks>: per (triple, block).  draw_tiles takes a span -- the words gone through and the rows kept of each:
//     the whole chromosome, or a segment's words with the same masks --; a word cut by a block boundary is read by both neighbours and
//     each keeps its own rows.  The same 3 x E histogram and bins; the workgroup writes its own 3 E partials, zeros for a segment
//     without a row.
//
// The expected counts per genome block (colate_topo_expected_blocks; count_topo.h: the expected counts) run the staging, planes, bins
// and segments, and nothing of the draws: no count kernel, no host wait, no rank and no stream of uniforms, since a row's addends
// depend on that row alone.
//   * topo_block_expected_kernel: one workgroup per (triple, block) over the segment's words; at every set bit of Q the two
//     fixed-point addends of expected_addends -- two 64-bit integer quotients, each a double first guess put right by its exact
//     integer remainder -- go into 64-bit LDS histograms, the row into a 32-bit one; the workgroup writes its 3 E integers as [E][3],
//     which the host copies into `counts` as they lie.  draw_tiles is not used.  No global atomics, no floating point in the result.
//
// THE HOST SIDE, behind the kernels: the four device calls share one call scope (TopoCall: range, counters, stream, timer, resident
// inputs, buffers, and last the wait on exit) with its stages -- stage_inputs: the resident upload, triples, epochs and planes;
// stage_ranks: counts, the one wait, bases, the stream's check, uniforms; stage_bins --, one chunk size (chunk_triples), one chunk loop
// (for_chunks) over a launch and a collect step of each call, and one launch of a grid per (triple, group) (launch_groups).  Nothing
// outside this file launches a kernel of it.
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

// The groups of a triple, in the genome's order: what one workgroup of the count and of the profile kernel takes, the kernels being
// written over "the words of a group".  groups(g): the chromosome of group g and its span.  The C chromosomes, each whole:
struct Chromosomes {
  struct Group {
    int c;
    WholeChromosome span;
  };
  __device__ __forceinline__ int G(const DeviceInputs& in) const { return in.C; }
  __device__ __forceinline__ Group operator()(int g) const { return Group{g, WholeChromosome()}; }
};
// ... or the nb blocks of this mode, each a segment of a chromosome's rows:
struct Blocks {
  int nb;
  const Segment* seg;
  struct Group {
    int c;
    SegmentWords span;
  };
  __device__ __forceinline__ int G(const DeviceInputs&) const { return nb; }
  __device__ __forceinline__ Group operator()(int g) const {
    const Segment sg = seg[g];
    return Group{sg.c, SegmentWords(sg)};
  }
};

// A triple at chromosome c: its three planes from the chromosome's first word -- Q is their conjunction --, the W words of the
// chromosome, and the index entries of its target and its reference from the chromosome's first row.
struct TripleAt {
  const unsigned long long *hT, *hR, *qC;
  const Idx *TI, *RI;
  long long W;
  __device__ __forceinline__ TripleAt(const DeviceInputs& in, int S, const Triple& t, int c, const unsigned long long* planes) {
    const long long w0 = in.word_off[c];
    W = in.word_off[c + 1] - w0;
    const long long r0 = in.row_off[c];
    hT = planes + (size_t)t.target * in.words + w0;
    hR = planes + (size_t)t.reference * in.words + w0;
    qC = planes + (size_t)(S + t.cond) * in.words + w0;
    TI = in.idx + (size_t)t.target * in.n + r0;
    RI = in.idx + (size_t)t.reference * in.n + r0;
  }
  __device__ __forceinline__ unsigned long long Q(long long k) const { return hT[k] & hR[k] & qC[k]; }
};

// One wave per (triple, group): popc(Q) over the group's words, the first and the last one of a segment masked; lane 0 writes
// cnt[p][g].  (Where `groups` stands in the two kernels' argument lists is chosen for the kernel arguments' layout: Blocks lies where
// nb and seg lay, and the empty Chromosomes in the profile kernel fills padding behind E, so that no other argument moves.)
template <class Groups>
__global__ __launch_bounds__(64) void topo_count_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                        const unsigned long long* __restrict__ planes, Groups groups, int* __restrict__ cnt) {
  const int G = groups.G(in), g = blockIdx.x % G, p = p0 + blockIdx.x / G;  // (triple p, group g)
  const int lane = threadIdx.x;
  const Triple t = triples[p];
  const auto group = groups(g);
  const TripleAt at(in, S, t, group.c, planes);
  int n = 0;
  for (long long k = group.span.first() + lane; k < group.span.end(at.W); k += 64) n += __popcll(at.Q(k) & group.span.keep(k));
  n = wave_sum(n);  // (a chromosome has fewer than 2^31 rows)
  if (lane == 0) cnt[(size_t)p * G + g] = n;
}

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
  const TripleAt at(in, S, t, c, planes);
  const long long W = span.end(at.W);
  for (long long tile0 = span.first(), tile = 0; tile0 < W; tile0 += kTileWords, tile++) {
    const long long k = tile0 + lane;
    const unsigned long long q = k < W ? at.Q(k) & span.keep(k) : 0ull;
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
          sign = draw_sign(at.TI[i], at.RI[i], u[2 * rank], u[2 * rank + 1]);
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

// One workgroup of kDrawWaves waves per (triple, group): the histogram zeroed behind a barrier, the draws over the group's words, a
// second barrier, and the workgroup's own 3 E words of `part`.  base: the rank of the group's first qualifying row; an empty segment
// goes through no word and writes zeros.  Both barriers are reached by every wave.
template <class Groups>
__global__ __launch_bounds__(kDrawWaves * 64) void topo_profile_kernel(DeviceInputs in, int S, int p0, const Triple* __restrict__ triples,
                                                                       const unsigned long long* __restrict__ planes,
                                                                       const long long* __restrict__ base, const double* __restrict__ u,
                                                                       const unsigned short* __restrict__ bin, int E, Groups groups,
                                                                       unsigned* __restrict__ part) {
  __shared__ unsigned hist[3 * kMaxProfileEpochs];
  const int G = groups.G(in), g = blockIdx.x % G, j = blockIdx.x / G;  // (triple p0 + j, group g)
  const auto group = groups(g);
  for (int i = threadIdx.x; i < 3 * E; i += kDrawWaves * 64) hist[i] = 0;
  __syncthreads();
  BinRows sink{bin + in.row_off[group.c], hist, E};
  draw_tiles(in, S, triples[p0 + j], group.c, base[(size_t)(p0 + j) * G + g], planes, u, sink, group.span);
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
  const TripleAt at(in, S, t, sg.c, planes);
  const unsigned short* const epoch_of = bin + in.row_off[sg.c];
  for (long long tile0 = span.w_first + (long long)wave * kTileWords; tile0 < span.w_end; tile0 += kDrawWaves * kTileWords) {
    const long long k = tile0 + lane;
    const unsigned long long q = k < span.w_end ? at.Q(k) & span.keep(k) : 0ull;
    for (unsigned long long left = __ballot(q != 0); left; left &= left - 1) {  // (alike in the whole wave)
      const int w = __builtin_ctzll(left);
      const unsigned long long qw = wave_uniform(__shfl(q, w, 64));
      if ((qw >> lane) & 1) {
        const long long i = (tile0 + w) * 64 + lane;  // (a set bit of Q is a row of the chromosome, and of the segment by the mask)
        const Addends x = expected_addends(at.TI[i], at.RI[i]);
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

// The four device calls of this file, and what each leaves for its two diagnostic getters: reset at the start of the call, set at
// its successful end.
enum Call { kSamples, kProfile, kProfileBlocks, kExpectedBlocks, kCalls };
struct Counters {
  int chunks = 0;
  double kernel_seconds = 0.0;
};
thread_local Counters g_counters[kCalls];

// bytes of what a chunk of triples leaves on the device -- the two output planes of colate_topo_samples, the partial histograms
// of the profile calls, the partial sums of the expected counts -- (COLATE_TOPO_BUDGET: bytes, for the tests)
long long output_budget() {
  if (const char* e = std::getenv("COLATE_TOPO_BUDGET")) return std::max(1LL, std::atoll(e));
  return 256LL << 20;
}

// Triples per chunk, where the budget and the grid bound meet: what a chunk leaves on the device, bytes_per_triple each, within the
// budget, and its G workgroups per triple within 2^31 - 1; one triple where its output alone is above the budget.
long long chunk_triples(long long P, long long bytes_per_triple, int G) {
  return std::max(1LL, std::min<long long>({P, output_budget() / std::max(1LL, bytes_per_triple), 0x7fffffffLL / G}));
}

// planes[2 S][words] of the resident inputs, whose arrays 0 .. S - 1 are the walk indices and S .. 2 S - 1 the cond indices
hipError_t planes_launch(const DeviceInputs& in, int S, unsigned long long* planes, hipStream_t stream) {
  if (in.words < 1 || in.S < 1) return hipSuccess;
  const long long blocks = (in.words + kPlaneTile / 64 - 1) / (kPlaneTile / 64);
  if (blocks > 0x7fffffffLL || in.S > 65535 || in.S != 2 * S) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_planes_kernel, dim3((unsigned)blocks, (unsigned)in.S), dim3(kPlaneTile), 0, stream, in, S, planes);
  return hipGetLastError();
}

// bin[n] = age_epoch of every searched row, the rows of all chromosomes back to back
hipError_t bins_launch(const DeviceInputs& in, int E, const double* epochs, unsigned short* bin, hipStream_t stream) {
  if (in.n < 1) return hipSuccess;
  const long long blocks = (in.n + kPlaneTile - 1) / kPlaneTile;
  if (blocks > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topo_bins_kernel, dim3((unsigned)blocks), dim3(kPlaneTile), 0, stream, in.rows, in.n, E, epochs, bin);
  return hipGetLastError();
}

// A kernel with one workgroup of `threads` per (triple, group) for the triples [p0, p1) of G groups each; E: the epochs it bins
// into (kNoEpochs: it bins nothing).  Refused: a grid above 2^31 - 1 workgroups, an E the histograms in LDS have no room for.
constexpr int kNoEpochs = 1;
template <class Kernel, class... Args>
int launch_groups(const char* what, Kernel kernel, int threads, int p0, int p1, int G, int E, hipStream_t stream, Args... args) {
  if (p1 <= p0 || G < 1) return COLATE_OK;
  const long long grid = (long long)(p1 - p0) * G;
  if (grid > 0x7fffffffLL || E < 1 || E > kMaxProfileEpochs) return hip_fail(hipErrorInvalidValue, what);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), 0, stream, args...);
  if (hipError_t e = hipGetLastError()) return hip_fail(e, what);
  return COLATE_OK;
}

// What every device call opens behind ensure_device(), in the order that is right for all of them: the profiler's range, the
// call's counters reset, the workspace with its stream (rc: what reserving it gave; the call returns it where it is not COLATE_OK),
// the timer, the resident inputs and the buffers of the call, the host arrays an asynchronous copy reads or writes, and last the
// guard that waits for the stream -- so that on every return path the stream is idle before any of those goes.  A host array of a
// call's own that a copy on the stream touches is declared in front of this object.
// The timer's intervals are opened and closed by kernels(true / false), so that a stage can launch into the interval the stage in
// front of it left open.
struct TopoCall {
  ProfRange range;
  Counters& counters;
  const int rc;
  const hipStream_t stream;  // (the workspace's stream: no second one)
  colate_iw::KernelTimer timer;
  bool timing = false;
  colate_iw::Resident res;
  DeviceBuffers buf;
  std::vector<const Idx*> both;  // the walk indices, then the cond indices
  std::vector<int> cnt;
  std::vector<long long> base, n;  // [P][G], [P]: the qualifying rows
  unsigned long long* d_planes = nullptr;
  Triple* d_triples = nullptr;
  int* d_cnt = nullptr;
  long long* d_base = nullptr;
  double *d_u = nullptr, *d_epochs = nullptr;
  unsigned short* d_bin = nullptr;
  int E = 0;
  const colate_iw::StreamSync sync_at_exit;

  TopoCall(Call which, const char* what)
      : range(what), counters(g_counters[which] = Counters()), rc(thread_workspace().reserve(256, 256)), stream(thread_workspace().stream),
        timer(stream), sync_at_exit{stream} {}

  int kernels(bool on) {
    if (on != timing) HIP_TRY(timer.mark());
    timing = on;
    return COLATE_OK;
  }

  // The inputs on the device and the planes launched, the timer's interval left open behind them: the walk and the cond indices
  // resident, the triples, the epochs of a call that bins (E > 0), and room for all that the stages behind this one fill -- the
  // counts and bases of stage_ranks over G groups per triple (G > 0), on the host and on the device, the rows' epochs of stage_bins --
  // so that nothing but launches falls between two kernels of one interval.
  int stage_inputs(const View& v, long long words, int G, int E_bins = 0, const double* epochs = nullptr) {
    both.resize((size_t)2 * v.S * v.C);
    std::copy_n(v.idx, (size_t)v.S * v.C, both.begin());
    std::copy_n(v.cidx, (size_t)v.S * v.C, both.begin() + (size_t)v.S * v.C);
    colate_iw::View iv;
    iv.C = v.C, iv.row_off = v.row_off, iv.rows = v.rows, iv.S = 2 * v.S, iv.idx = both.data(), iv.M = 0, iv.P = 0, iv.pairs = nullptr, iv.nbpb = 1;
    if (int e = res.upload(iv, stream)) return e;
    E = E_bins;
    HIP_TRY(buf.device(d_planes, (size_t)2 * v.S * (size_t)words)); HIP_TRY(buf.device(d_triples, (size_t)v.P));
    if (G > 0) {
      const size_t PG = (size_t)v.P * (size_t)G;
      cnt.resize(PG), base.resize(PG), n.assign((size_t)v.P, 0);
      HIP_TRY(buf.device(d_cnt, PG)); HIP_TRY(buf.device(d_base, PG));
    }
    if (E > 0) {
      HIP_TRY(buf.device(d_bin, (size_t)v.row_off[v.C])); HIP_TRY(buf.device(d_epochs, (size_t)E));
    }
    HIP_TRY(colate_iw::h2d(stream, d_triples, v.triples, sizeof(Triple) * (size_t)v.P));
    HIP_TRY(colate_iw::h2d(stream, d_epochs, epochs, sizeof(double) * (size_t)E));
    if (int e = kernels(true)) return e;
    if (hipError_t e = planes_launch(res.in, v.S, d_planes, stream)) return hip_fail(e, "topo planes kernel launch");
    return COLATE_OK;
  }

  // A triple's groups as the kernels take them: the chromosomes need nothing staged; the blocks are the view's segments on the device
  int stage_groups(const std::vector<Segment>*, Chromosomes&) { return COLATE_OK; }
  int stage_groups(const std::vector<Segment>* seg, Blocks& blocks) {
    Segment* d_seg = nullptr;
    HIP_TRY(buf.device(d_seg, seg->size()));
    HIP_TRY(colate_iw::h2d(stream, d_seg, seg->data(), sizeof(Segment) * seg->size()));
    blocks = Blocks{(int)seg->size(), d_seg};
    return COLATE_OK;
  }

  // Behind stage_inputs: the counts per (triple, group) into its interval, the one host wait for them, every group's first rank --
  // the groups in the genome's order: a group's base is the sum of the groups in front --, the stream checked, and the uniforms the
  // longest triple needs.
  template <class Groups>
  int stage_ranks(const View& v, const Groups& groups, int G, const char* what) {
    const size_t PG = (size_t)v.P * (size_t)G;
    const long long grid_most = 0x7fffffffLL / G;
    for (long long p0 = 0; p0 < v.P; p0 += grid_most)
      if (int e = launch_groups(what, topo_count_kernel<Groups>, 64, (int)p0, (int)std::min<long long>(v.P, p0 + grid_most), G, kNoEpochs, stream,
                                res.in, v.S, (int)p0, d_triples, d_planes, groups, d_cnt))
        return e;
    if (int e = kernels(false)) return e;
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * PG, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the one wait for the counts
    long long most = 0;
    for (int p = 0; p < v.P; p++) {
      for (int g = 0; g < G; g++) base[(size_t)p * G + g] = n[(size_t)p], n[(size_t)p] += cnt[(size_t)p * G + g];
      most = std::max(most, n[(size_t)p]);
    }
    if (int e = check_stream(v, n.data())) return e;
    // every triple starts from the run's seed: one stream for all, as long as the longest needs
    HIP_TRY(buf.device(d_u, (size_t)(2 * most)));
    HIP_TRY(colate_iw::h2d(stream, d_u, v.uniforms, sizeof(double) * (size_t)(2 * most)));
    HIP_TRY(colate_iw::h2d(stream, d_base, base.data(), sizeof(long long) * PG));
    return COLATE_OK;
  }

  // Every searched row's epoch, once for every triple: into the interval stage_inputs left open, or one of its own
  int stage_bins() {
    if (int e = kernels(true)) return e;
    if (hipError_t e = bins_launch(res.in, E, d_epochs, d_bin, stream)) return hip_fail(e, "topo bins kernel launch");
    return kernels(false);
  }

  // The chunks of `chunk` triples each: launch(p0, p1) between two marks of the timer, then collect(p0, p1), which takes the chunk's
  // output off the device before the next launch overwrites it (one stream), and the chunk counted.
  template <class Launch, class Collect>
  int for_chunks(long long P, long long chunk, Launch&& launch, Collect&& collect) {
    for (long long p0 = 0; p0 < P; p0 += chunk) {
      const long long p1 = std::min(P, p0 + chunk);
      if (int e = kernels(true)) return e;
      if (int e = launch((int)p0, (int)p1)) return e;
      if (int e = kernels(false)) return e;
      if (int e = collect(p0, p1)) return e;
      counters.chunks++;
    }
    return COLATE_OK;
  }

  // the call's successful end, the stream idle
  int done() {
    counters.kernel_seconds = timer.seconds();
    return COLATE_OK;
  }
};

// What the grids refuse of a view: the plane kernel's and the count kernel's, and with `binned` the bins kernel's.
int check_grids_of(const View& v, bool binned) {
  if (2LL * v.S > 65535) return fail(COLATE_ELIMIT, "S=%d above the grid of the plane kernel (32767)", v.S);
  if ((long long)v.P * v.C > 0x7fffffffLL) return fail(COLATE_ELIMIT, "P x C = %lld above the grid of the count kernel", (long long)v.P * v.C);
  if (binned && (v.row_off[v.C] + kPlaneTile - 1) / kPlaneTile > 0x7fffffffLL)
    return fail(COLATE_ELIMIT, "%lld rows above the grid of the bins kernel", v.row_off[v.C]);
  return COLATE_OK;
}

}  // namespace

namespace colate_topo {

int topo_view_device(const View& v, long long cap, long long* word_off, unsigned long long* plus, unsigned long long* minus, long long* draws) {
  if (int rc = check_outputs(cap, word_off, plus, minus, draws)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = check_grids_of(v, false)) return rc;
  std::vector<long long> woff((size_t)v.C + 1);
  const long long words = colate_iw::mask_words(v.C, v.row_off, woff.data());
  if (int rc = check_capacity(v.P, words, cap)) return rc;
  if (int rc = ensure_device()) return rc;
  TopoCall call(kSamples, "colate_topo_samples: H2D + planes + counts; the uniforms; per chunk of triples the draws + D2H");
  if (call.rc) return call.rc;
  const hipStream_t stream = call.stream;
  const long long chunk = chunk_triples(v.P, 2 * words * (long long)sizeof(unsigned long long), v.C);  // the two output planes
  unsigned long long *d_plus = nullptr, *d_minus = nullptr;
  HIP_TRY(call.buf.device(d_plus, (size_t)(chunk * words))); HIP_TRY(call.buf.device(d_minus, (size_t)(chunk * words)));
  if (int rc = call.stage_inputs(v, words, v.C)) return rc;
  if (int rc = call.stage_ranks(v, Chromosomes(), v.C, "topo count kernel launch")) return rc;
  const int rc = call.for_chunks(
      v.P, chunk,
      [&](int p0, int p1) {
        return launch_groups("topo draw kernel launch", topo_draw_kernel, kDrawWaves * 64, p0, p1, v.C, kNoEpochs, stream, call.res.in, v.S, p0,
                             call.d_triples, call.d_planes, call.d_base, call.d_u, d_plus, d_minus);
      },
      [&](long long p0, long long p1) {
        const size_t bytes = sizeof(unsigned long long) * (size_t)((p1 - p0) * words);
        if (bytes) {
          HIP_TRY(hipMemcpyAsync(plus + p0 * words, d_plus, bytes, hipMemcpyDeviceToHost, stream));
          HIP_TRY(hipMemcpyAsync(minus + p0 * words, d_minus, bytes, hipMemcpyDeviceToHost, stream));
        }
        return (int)COLATE_OK;
      });
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(draws, call.n.data(), sizeof(long long) * (size_t)v.P);
  std::memcpy(word_off, woff.data(), sizeof(long long) * woff.size());
  return call.done();
}

namespace {

// What the two profile calls do behind their checks, over the groups of a triple -- its chromosomes, or the blocks in `seg` --:
// per chunk of triples the binned draws into the partial histograms, 12 E bytes per (triple, group), the wait for them, and
// collect(p0, p1, part), which forms `counts` from the chunk's part[(p - p0) * G + g][3][E].
template <class Groups, class Collect>
int profile_device(Call which, const char* range, const char* count_what, const char* profile_what, const View& v, int E, const double* epochs,
                   int G, const std::vector<Segment>* seg, long long* draws, Collect&& collect) {
  const long long words = colate_iw::mask_words(v.C, v.row_off, nullptr);
  if (int rc = ensure_device()) return rc;
  const size_t per_group = 3 * (size_t)E;
  const long long chunk = chunk_triples(v.P, (long long)(per_group * sizeof(unsigned)) * G, G);
  std::vector<unsigned> part((size_t)chunk * (size_t)G * per_group);
  TopoCall call(which, range);
  if (call.rc) return call.rc;
  const hipStream_t stream = call.stream;
  unsigned* d_part = nullptr;
  HIP_TRY(call.buf.device(d_part, part.size()));
  Groups groups{};
  if (int rc = call.stage_groups(seg, groups)) return rc;
  if (int rc = call.stage_inputs(v, words, G, E, epochs)) return rc;
  if (int rc = call.stage_ranks(v, groups, G, count_what)) return rc;
  if (int rc = call.stage_bins()) return rc;
  const int rc = call.for_chunks(
      v.P, chunk,
      [&](int p0, int p1) {
        return launch_groups(profile_what, topo_profile_kernel<Groups>, kDrawWaves * 64, p0, p1, G, E, stream, call.res.in, v.S, p0, call.d_triples,
                             call.d_planes, call.d_base, call.d_u, call.d_bin, E, groups, d_part);
      },
      [&](long long p0, long long p1) {
        HIP_TRY(hipMemcpyAsync(part.data(), d_part, sizeof(unsigned) * (size_t)(p1 - p0) * (size_t)G * per_group, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // (the one wait at the end where one chunk holds every triple)
        collect(p0, p1, part.data());
        return (int)COLATE_OK;
      });
  if (rc) return rc;
  std::memcpy(draws, call.n.data(), sizeof(long long) * (size_t)v.P);
  return call.done();
}

}  // namespace

int topo_profile_device(const View& v, int E, const double* epochs, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  if (int rc = check_grids_of(v, true)) return rc;
  const size_t per_group = 3 * (size_t)E;
  return profile_device<Chromosomes>(
      kProfile, "colate_topo_profile: H2D + planes + counts + bins; the uniforms; per chunk of triples the binned draws + D2H",
      "topo count kernel launch", "topo profile kernel launch", v, E, epochs, v.C, nullptr, draws, [&](long long p0, long long p1, const unsigned* part) {
        for (long long p = p0; p < p1; p++) {  // a triple's [E][3]: the chromosomes' [3][E] partials, summed in long long
          long long* const out = counts + (size_t)p * per_group;
          std::fill_n(out, per_group, 0LL);
          for (int c = 0; c < v.C; c++) {
            const unsigned* const h = part + ((size_t)(p - p0) * v.C + c) * per_group;
            for (int e = 0; e < E; e++) out[3 * e] += h[e], out[3 * e + 1] += h[E + e], out[3 * e + 2] += h[2 * E + e];
          }
        }
      });
}

int topo_profile_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts, long long* draws) {
  if (!counts || !draws) return fail(COLATE_EINVAL, "NULL pointer argument");
  if (int rc = check_epochs(E, epochs)) return rc;
  if (int rc = check_view(v)) return rc;
  std::vector<int> blk_off;
  if (int rc = check_blocks(v, E, nbpb, nb, blk_off)) return rc;
  if (int rc = check_grids_of(v, true)) return rc;
  std::vector<Segment> seg((size_t)nb);
  block_segments(v, nbpb, blk_off.data(), seg.data());
  const size_t per_group = 3 * (size_t)E;
  // the counts per (triple, block) take the place of those per (triple, chromosome)
  return profile_device<Blocks>(
      kProfileBlocks,
      "colate_topo_profile_blocks: H2D + planes + block counts + bins; the uniforms; per chunk of triples the binned draws of every block + D2H",
      "topo block count kernel launch", "topo block profile kernel launch", v, E, epochs, nb, &seg, draws,
      [&](long long p0, long long p1, const unsigned* part) {
        for (size_t k = 0; k < (size_t)(p1 - p0) * (size_t)nb; k++) {  // every (triple, block) owns its partials: [3][E] into [E][3]
          const unsigned* const h = part + k * per_group;
          long long* const out = counts + ((size_t)p0 * (size_t)nb + k) * per_group;
          for (int e = 0; e < E; e++) out[3 * e] = h[e], out[3 * e + 1] = h[E + e], out[3 * e + 2] = h[2 * E + e];
        }
      });
}

int topo_expected_blocks_device(const View& v, int E, const double* epochs, int nbpb, int nb, long long* counts) {
  std::vector<int> blk_off;
  if (int rc = check_expected(v, E, epochs, nbpb, nb, counts, blk_off)) return rc;
  if (int rc = check_grids_of(v, true)) return rc;
  const long long words = colate_iw::mask_words(v.C, v.row_off, nullptr);
  std::vector<Segment> seg((size_t)nb);
  block_segments(v, nbpb, blk_off.data(), seg.data());
  if (int rc = ensure_device()) return rc;
  TopoCall call(kExpectedBlocks, "colate_topo_expected_blocks: H2D + planes + bins; per chunk of triples the expected counts of every block + D2H");
  if (call.rc) return call.rc;
  const hipStream_t stream = call.stream;
  const size_t per_group = 3 * (size_t)E;
  const long long chunk = chunk_triples(v.P, (long long)(per_group * sizeof(long long)) * nb, nb);  // 24 E bytes per (triple, block)
  long long* d_part = nullptr;
  HIP_TRY(call.buf.device(d_part, (size_t)chunk * (size_t)nb * per_group));
  Blocks blocks{};
  if (int rc = call.stage_groups(&seg, blocks)) return rc;
  // nothing of the draws: no count pass, no rank, no uniform, and so no wait in front of the chunks
  if (int rc = call.stage_inputs(v, words, 0, E, epochs)) return rc;
  if (int rc = call.stage_bins()) return rc;
  const int rc = call.for_chunks(
      v.P, chunk,
      [&](int p0, int p1) {
        return launch_groups("topo block expected kernel launch", topo_block_expected_kernel, kDrawWaves * 64, p0, p1, nb, E, stream, call.res.in, v.S,
                             p0, call.d_triples, call.d_planes, blocks.nb, blocks.seg, call.d_bin, E, d_part);
      },
      [&](long long p0, long long p1) {  // every (triple, block) owns its partials, written as [E][3]: they are `counts` as they lie
        HIP_TRY(hipMemcpyAsync(counts + (size_t)p0 * (size_t)nb * per_group, d_part, sizeof(long long) * (size_t)(p1 - p0) * (size_t)nb * per_group,
                               hipMemcpyDeviceToHost, stream));
        return (int)COLATE_OK;
      });
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(stream));  // the one wait of the call
  return call.done();
}

}  // namespace colate_topo

extern "C" {
int colate_topo_samples_chunks(void) { return g_counters[kSamples].chunks; }
double colate_topo_samples_kernel_seconds(void) { return g_counters[kSamples].kernel_seconds; }
int colate_topo_profile_chunks(void) { return g_counters[kProfile].chunks; }
double colate_topo_profile_kernel_seconds(void) { return g_counters[kProfile].kernel_seconds; }
int colate_topo_profile_blocks_chunks(void) { return g_counters[kProfileBlocks].chunks; }
double colate_topo_profile_blocks_kernel_seconds(void) { return g_counters[kProfileBlocks].kernel_seconds; }
int colate_topo_expected_blocks_chunks(void) { return g_counters[kExpectedBlocks].chunks; }
double colate_topo_expected_blocks_kernel_seconds(void) { return g_counters[kExpectedBlocks].kernel_seconds; }
}
