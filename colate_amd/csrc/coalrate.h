// colate_amd/csrc/coalrate.h -- `CoalRate --mode local_ancestry` inside libcolate_amd.so (coal_LA::populate,
// include/coal/coal_tree.cpp:447-527): what the host side (coalrate.cpp: preparation of the calls, host twin, driver) and
// the device side (coalrate_kernel.hip) share.  DESIGN.md ("CoalRate") derives the count formulation used here.
//
// One call = one tree with a weight w, a group vector s and a block.  Per (group pair gp = {g1 >= g2}, epoch e) it adds
//   num   += B * wq                                              wq = w / 1e9
//   denom += ((K * width[e] + R) * wq) - sub * wq
// with B the leaf pairs of gp whose MRCA lies in epoch e, R the sum over those MRCAs v, ordered by (epoch, label), of
// m_v * (t_v - epochs[e]) (m_v: the pairs of gp meeting at v), K = cumA - cumB the pairs that cross the whole of e (cumA:
// the pairs of gp whose older sample has its age in an epoch <= e, a table per group vector; cumB: the pairs coalesced in
// an epoch <= e) and sub the pairs' sum of (age - epochs[e_age]) in epoch e (a table per group vector).  All counts are
// exact integers; every double sum has the one order written here, for the kernel and the host twin alike.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "colate_amd.h"
#include "colate_internal.h"
#include "condcoal.h"

#if defined(__HIPCC__)
#define CR_HD __host__ __device__ __forceinline__
#else
#define CR_HD inline
#endif

namespace colate_cr {

using colate_cc::kMaxHaplotypes;  // (pair counts per node stay below 2^27, per call below 2^28: int32, exact in double)

// An internal node of a prepared call: the DFS leaf ranges [lo, mid) and [mid, hi) of its two children, its epoch and
// t_v - epochs[ev].
struct CrNode {
  unsigned short lo, mid, hi, ev;
  double dt;
};
static_assert(sizeof(CrNode) == 16, "one 16-byte load per node");

// What every call of a run shares.
struct CrRun {
  int N = 0, G = 0, S = 0;
  std::vector<double> epochs;  // [E]
  std::vector<double> ages;    // [N] or empty (modern samples)
  std::vector<int> groups;     // [S][N] group vectors
  int E() const { return (int)epochs.size(); }
  int GP() const { return G * (G + 1) / 2; }
};

// group pair index of g1 >= g2
CR_HD int cr_pair(int g1, int g2) { return g1 * (g1 + 1) / 2 + g2; }

// The per-group-vector tables: over the occupied age epochs oa (ascending), the pairs of each group pair whose older
// sample's age lies there, and their sum of (age - epochs[epoch]).  Modern samples: one occupied epoch, 0, without sums.
struct CrTables {
  int OA = 0;
  std::vector<int> oa_epoch;        // [OA]
  std::vector<long long> pairs;     // [S][OA][GP]
  std::vector<double> sub;          // [S][OA][GP]
  std::vector<double> width;        // [E]: epochs[e+1] - epochs[e], 0 for the last
};
// False with a message when a group label or an age is out of range.
bool make_tables(const CrRun& run, CrTables& tab, std::string& err);

// A chunk of prepared calls, back to back.
struct CrChunk {
  int N = 0, T = 0;
  std::vector<int> leaf;     // [T][N] DFS leaf order
  std::vector<CrNode> node;  // [T][N-1] internal nodes by (epoch, label)
  std::vector<double> w;     // [T]
  std::vector<int> gv, block;
  void clear() {
    T = 0;
    leaf.clear(), node.clear(), w.clear(), gv.clear(), block.clear();
  }
  int append(int n);  // room for one more call; returns its index
  // a copy of call k of `src` at the end (a tree makes one call per local-ancestry segment it reaches); returns its index
  int append_from(const CrChunk& src, int k);
};

// Call k of the chunk from a raw tree (Relate labelling): checks it (colate_cc::prepare_tree), dates its nodes as
// Tree::GetCoordinates does (float), finds their epochs and sorts them.  False with a message for a malformed tree, a
// node older than the last epoch boundary, or a node in an epoch below that of a sample age under it.
bool prepare_call(const CrRun& run, const int* parent, const double* bl, CrChunk& c, int k, std::string& err);

// One lane's walk over the nodes of a call for one group pair: cumB[e * stride] and R[e * stride] for every epoch.
// pre(g, q): the leaves of group g among the first q of the leaf order.
template <class Pre>
CR_HD void cr_count_pair(int nodes, int E, const CrNode* node, int g1, int g2, Pre pre, int* cumB, double* R, size_t stride) {
  int cur = 0, b = 0, cum = 0;
  double r = 0.0;
  for (int j = 0; j < nodes; j++) {
    const CrNode nd = node[j];
    while (cur < (int)nd.ev) {
      cum += b;
      cumB[cur * stride] = cum;
      R[cur * stride] = r;
      b = 0, r = 0.0, cur++;
    }
    const int l1 = pre(g1, nd.mid) - pre(g1, nd.lo), r1 = pre(g1, nd.hi) - pre(g1, nd.mid);
    int m;
    if (g1 == g2) {
      m = l1 * r1;
    } else {
      const int l2 = pre(g2, nd.mid) - pre(g2, nd.lo), r2 = pre(g2, nd.hi) - pre(g2, nd.mid);
      m = l1 * r2 + l2 * r1;
    }
    b += m;
    r += (double)m * nd.dt;
  }
  while (cur < E) {
    cum += b;
    cumB[cur * stride] = cum;
    R[cur * stride] = r;
    b = 0, r = 0.0, cur++;
  }
}

// One call's addends of cell (e, gp): cb / cb_prev = cumB[e] / cumB[e-1] (0 at e = 0), ca = cumA[e], sub = the table's
// entry where e is an occupied age epoch (0 otherwise).
CR_HD void cr_fold_cell(int cb, int cb_prev, long long ca, double r, double sub, double width, double w, double& num, double& den) {
  const double wq = w / 1e9;
  num += (double)(cb - cb_prev) * wq;
  double d = (double)(ca - (long long)cb) * width;
  d = d + r;
  d = d * wq;
  d = d - sub * wq;
  den += d;
}

// Per-block sums of a run: num / denom [block][E][GP].
struct CrSums {
  int blocks = 0;
  std::vector<double> num, den;
};

// One way to accumulate, for both CoalRate modes (Chunk: CrChunk here, colate_crt::CrtChunk for --mode tree): the prepared
// calls go in chunk by chunk, the per-block sums come out.  A mode's two implementations sum in the same order (here: per
// call and group pair over the nodes by (epoch, label); per cell over the calls in input order), so their sums agree bit
// for bit.
template <class Chunk>
class BlockSumWalker {
 public:
  virtual ~BlockSumWalker() = default;
  virtual bool submit(const Chunk& c) = 0;
  virtual bool finish(CrSums& out) = 0;
  const std::string& error() const { return err_; }
  int error_code() const { return code_; }
  double gpu_seconds() const { return gpu_s_; }  // kernel time by events (0 for the host twin)

 protected:
  bool fail(const std::string& what, int code) {
    err_ = what;
    code_ = code;
    return false;
  }
  double gpu_s_ = 0;

 private:
  std::string err_;
  int code_ = 0;
};
using CoalRateWalker = BlockSumWalker<CrChunk>;

std::unique_ptr<CoalRateWalker> make_host_walker(const CrRun& run, const CrTables& tab);
// Null, the reason in `why` and its COLATE_E code in *code, when there is no device or the run does not fit it (device -1:
// the calling thread's).
std::unique_ptr<CoalRateWalker> make_device_walker(int device, const CrRun& run, const CrTables& tab, int max_calls, std::string& why,
                                                   int* code = nullptr);
// What the first-kernel launches of the calling thread's last device call of a mode looked like (diagnostics:
// colate_coalrate_launch_shape, colate_coalrate_tree_launch_shape).  The C ABI's device entry resets it, the device walker's
// launch() notes every launch; all 0 after a call that launched nothing.
struct LaunchStats {
  int launches = 0, cpw_min = 0, cpw_max = 0, lpc = 0, lds = 0;
  void note(int cpw, int lanes_per_call, bool in_lds) {
    cpw_min = launches ? std::min(cpw_min, cpw) : cpw;
    cpw_max = launches ? std::max(cpw_max, cpw) : cpw;
    lpc = lanes_per_call, lds = in_lds ? 1 : 0;
    launches++;
  }
  int report(int* out) const {  // out[5] (or null); returns the launches
    if (out) out[0] = launches, out[1] = cpw_min, out[2] = cpw_max, out[3] = lpc, out[4] = lds;
    return launches;
  }
};
enum LaunchMode { kLaunchLocalAncestry = 0, kLaunchTree = 1 };
LaunchStats& launch_stats(LaunchMode mode);  // the calling thread's

// device bytes per call of a chunk
size_t device_call_bytes(int N, int G, int E);
// Calls per chunk: the most that fit 4M node entries and 256 MiB of device memory, or COLATE_COALRATE_CHUNK_TREES where
// that is set and smaller (tests cross chunk and block boundaries on small inputs).
int chunk_calls_for(int N, int G, int E);


// What the C ABI bodies of the two modes share (colate_coalrate_accumulate[_host], colate_coalrate_tree_accumulate[_host]):
// the arguments both take, the checks both make, and the run itself.  A body makes the checks in its own order between
// those of its own; every message starts with `name`.
struct BlockAccumulate {
  const char* name;  // "coalrate" / "coalrate tree"
  bool device;
  int N, T;
  const double* weights;
  const int* blocks;
  int num_blocks, E;
  const double* epochs;

  int check_N() const {
    if (N < 2 || N > kMaxHaplotypes)
      return colate::fail(N < 2 ? COLATE_EINVAL : COLATE_ELIMIT, "%s: N = %d haplotypes (supported: 2 .. %d)", name, N, kMaxHaplotypes);
    return COLATE_OK;
  }
  // the epochs; then per tree its block, what extra(t) checks (COLATE_OK or a failure's code) and its weight
  template <class Extra>
  int check_trees(Extra extra) const {
    for (int e = 0; e < E; e++)
      if ((e == 0 && epochs[0] != 0.0) || (e && !(epochs[e] > epochs[e - 1])))
        return colate::fail(COLATE_EINVAL, "%s: epochs must start at 0 and increase", name);
    for (int t = 0; t < T; t++) {
      if (blocks[t] < 0 || blocks[t] >= num_blocks) return colate::fail(COLATE_EINVAL, "%s: tree %d in block %d", name, t, blocks[t]);
      if (const int rc = extra(t)) return rc;
      if (!std::isfinite(weights[t])) return colate::fail(COLATE_EINVAL, "%s: tree %d has weight %g", name, t, weights[t]);
    }
    return COLATE_OK;
  }
  // The sums over all trees: make(chunk, err, code) opens the device walker or the host twin for chunks of `chunk`
  // calls; prepare(t, c, err) appends tree t to the chunk, or leaves it out.
  template <class Chunk, class Make, class Prepare>
  int run(int chunk_calls, Make make, Prepare prepare, CrSums& sums) const {
    if (device && colate_device_count() <= 0) return colate::fail(COLATE_ENODEVICE, "%s: no usable HIP device", name);
    const int chunk = std::max(1, std::min(std::max(T, 1), chunk_calls));
    int code = 0;
    std::string err;
    std::unique_ptr<BlockSumWalker<Chunk>> w = make(chunk, err, &code);
    if (!w) return colate::fail(code ? code : COLATE_EHIP, "%s: %s", name, err.c_str());
    const auto walker_failed = [&] { return colate::fail(w->error_code() ? w->error_code() : COLATE_EHIP, "%s", w->error().c_str()); };
    Chunk c;
    for (int t0 = 0; t0 < T; t0 += chunk) {
      c.clear();
      const int t1 = std::min(T, t0 + chunk);
      for (int t = t0; t < t1; t++)
        if (!prepare(t, c, err)) return colate::fail(COLATE_EINVAL, "%s: tree %d: %s", name, t, err.c_str());
      if (!w->submit(c)) return walker_failed();
    }
    if (!w->finish(sums)) return walker_failed();
    return COLATE_OK;
  }
};

}  // namespace colate_cr
