// colate_amd/csrc/condcoal_walk.hpp -- the tree walk of `Colate --mode CondCoalRates` (include/coal/coal.cpp:4786-4999,
// GetConditionalCoalescentRate), one focal haplotype at a time, shared by the device kernel (condcoal_kernel.hip) and
// the host twin (condcoal.cpp): the same source, so the same float arithmetic on both sides.
//
// The reference walks, for every (focal f, conditional c != f) pair, from f to the root; once it has passed the
// ancestor a where c joins f's lineage (coal_age = the height of a), every member x of the sibling subtree met at
// each later step adds, for the step's height `coord`, the epoch pieces of [lower_age, coord) to denom and `factor` to
// num, in the row (focal epoch, epoch, group of x).  Two factorisations make that one walk per focal leaf:
//   * all conditionals that join f at the same ancestor a_k see the same addends: one class per such ancestor,
//     weighted by m_k, their number (an integer count times a float addend is exact in double);
//   * modern path (no sample ages): all members of a sibling subtree share the addends and differ only in group, so
//     the per-group counts of the subtree (prefix sums over one DFS leaf order per tree) replace the member loop.
// The ancient path keeps the member loop (lower_age depends on the member's sample age).  Every float quantity of the
// reference (coord, coal_age, lower_age, the epochs, each addend) is computed as there, operand for operand; only the
// summation is in double and in another order.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define CC_HD __host__ __device__
#else
#define CC_HD
#endif

namespace colate_cc {

// One prepared tree (2N-1 nodes, leaves 0..N-1, root 2N-2), and what every walk of the run shares.
struct CcTree {
  const int* parent;     // [2N-1], -1 at the root
  const double* bl;      // [2N-1] branch length above each node
  const int* lo;         // [2N-1] leaf range [lo, hi) of the node's subtree in the tree's DFS leaf order
  const int* hi;
  const int* leaf;       // [N] DFS leaf order: position -> haplotype
  const int* prefix;     // [G+1][N+1] per group (row G: the conditional group) count of haplotypes before a position
  float factor;          // the tree's weight (num_bases_tree_persists as float, or -1 for the extra pass of the last tree)
};

struct CcShared {
  int N, G, E, EF;
  const int* group;      // [N] group index of each haplotype
  const unsigned char* is_cond;  // [N]
  int cond_empty;        // the conditional group is empty: one virtual conditional (coal.cpp: conditional_haps = {-1})
  const double* ages;    // [N] sample ages, or nullptr (modern path)
  const float* epochs;   // [E]
  const float* efocal;   // [EF]
};

// accumulator layout: num at ((s * E + e) * G + g), denom at EF * E * G + the same
CC_HD inline int cc_slots(const CcShared& sh) { return 2 * sh.EF * sh.E * sh.G; }

// epoch[E] reads as +inf: the reference reads one past its vector there (a coordinate older than the last boundary)
CC_HD inline float cc_epoch_next(const CcShared& sh, int ep) {
  return ep + 1 < sh.E ? sh.epochs[ep + 1] : __builtin_inff();
}

// coal.cpp:4845-4851 / 4958-4964: the epoch a coalescence age starts in
CC_HD inline int cc_ep_init(const CcShared& sh, float coal_age) {
  int ep = 0;
  if (coal_age > sh.epochs[0]) {
    while (ep < sh.E && coal_age > sh.epochs[ep]) ep++;
    ep--;
  }
  return ep;
}

// Adds one class (weight m) of focal leaf f, which starts at node a with coal_age = coord (the height of a as the
// reference accumulates it), from the step above a up to the root.  `Acc` is add(slot, value) for the caller's storage.
template <class Acc>
CC_HD inline void cc_class_walk(const CcShared& sh, const CcTree& t, int f, int a, float coord, int s_class, double m,
                                Acc& acc) {
  const int root = 2 * sh.N - 2;
  const int NS = sh.EF * sh.E * sh.G;
  const float coal_age = coord;
  const float factor = t.factor;
  const int ep_init = cc_ep_init(sh, coal_age);
  const double age_f = sh.ages ? sh.ages[f] : 0.0;
  int node = a;
  for (;;) {
    coord = (float)((double)coord + t.bl[node]);  // coal.cpp:4839 `coord += node.branch_length` (float += double)
    const int p = t.parent[node];
    // the sibling's leaf range: the part of p's range that is not node's
    const int slo = (t.lo[node] == t.lo[p]) ? t.hi[node] : t.lo[p];
    const int shi = (t.lo[node] == t.lo[p]) ? t.hi[p] : t.lo[node];
    if (!sh.ages) {
      // modern (coal.cpp:4856-4867): every member has lower_age = coal_age, ep = ep_init.  A sibling subtree with fewer
      // members than there are groups is taken member by member, a larger one group by group (per-group counts).
      const bool by_member = shi - slo < sh.G;
      auto add_all = [&](int base, float v) {
        if (by_member) {
          for (int q = slo; q < shi; q++) acc.add(base + sh.group[t.leaf[q]], m * (double)v);
        } else {
          for (int g = 0; g < sh.G; g++) {
            const int cnt = t.prefix[g * (sh.N + 1) + shi] - t.prefix[g * (sh.N + 1) + slo];
            if (cnt) acc.add(base + g, m * (double)cnt * (double)v);
          }
        }
      };
      float lower = coal_age;
      int ep = ep_init;
      while (coord > cc_epoch_next(sh, ep)) {
        add_all(NS + (s_class * sh.E + ep) * sh.G, factor * (sh.epochs[ep + 1] - lower));
        ep++;
        lower = sh.epochs[ep];
      }
      add_all(NS + (s_class * sh.E + ep) * sh.G, factor * (coord - lower));
      add_all((s_class * sh.E + ep) * sh.G, factor);
    } else {
      // ancient (coal.cpp:4956-4992): per member
      for (int q = slo; q < shi; q++) {
        const int x = t.leaf[q];
        const double ax = sh.ages[x];
        float lower = (float)(age_f > ax ? age_f : ax);  // std::max(age, sample_ages[x]) into a float
        lower = lower > coal_age ? lower : coal_age;     // std::max(lower_age, coal_age)
        int s = s_class, ep = ep_init;
        if (!(lower <= coal_age)) {
          if (sh.efocal[s] < lower) {
            while (sh.efocal[s] < lower) {
              s++;
              if (s == sh.EF) break;
            }
            s--;
          }
          if (sh.epochs[ep] < lower) {
            while (sh.epochs[ep] < lower) {
              ep++;
              if (ep == sh.E) break;
            }
            ep--;
          }
        }
        while (coord > cc_epoch_next(sh, ep)) {
          const float piece = factor * (sh.epochs[ep + 1] - lower);
          acc.add(NS + (s * sh.E + ep) * sh.G + sh.group[x], m * (double)piece);
          ep++;
          lower = sh.epochs[ep];
        }
        const float piece = factor * (coord - lower);
        acc.add(NS + (s * sh.E + ep) * sh.G + sh.group[x], m * (double)piece);
        acc.add((s * sh.E + ep) * sh.G + sh.group[x], m * (double)factor);
      }
    }
    node = p;
    if (node == root) break;
  }
}

// The whole contribution of focal leaf f to one tree's accumulators, with the conditional group's prefix row `cpre`
// ([N+1]) and `self` = 1 if f is itself a conditional (neither is read when sh.cond_empty).
template <class Acc>
CC_HD inline void cc_focal_walk_cond(const CcShared& sh, const CcTree& t, int f, const int* cpre, int self, Acc& acc) {
  const int root = 2 * sh.N - 2;
  float coord = sh.ages ? (float)sh.ages[f] : 0.0f;
  if (sh.cond_empty) {  // one virtual conditional, in use from the start, focal epoch 0
    cc_class_walk(sh, t, f, f, coord, 0, 1.0, acc);
    return;
  }
  int prev = 0;  // conditionals below the previous node of the path, f itself excluded
  int node = f;
  for (;;) {
    const int cc = cpre[t.hi[node]] - cpre[t.lo[node]] - self;
    const int m = cc - prev;
    prev = cc;
    if (m > 0) {
      // the focal epoch of the class (coal.cpp:4814-4822: `<=`, modern; 4906-4913: `<`, ancient)
      int s = 0;
      if (!sh.ages) {
        if (sh.efocal[0] <= coord) {
          while (sh.efocal[s] <= coord) {
            s++;
            if (s == sh.EF) break;
          }
          if (s > 0) s--;
        }
      } else {
        if (sh.efocal[0] < coord) {
          while (sh.efocal[s] < coord) {
            s++;
            if (s == sh.EF) break;
          }
          s--;
        }
      }
      cc_class_walk(sh, t, f, node, coord, s, (double)m, acc);
    }
    coord = (float)((double)coord + t.bl[node]);
    node = t.parent[node];
    if (node == root) break;  // (coal.cpp:4871: the root itself is never tested, so its conditionals are not used)
  }
}

// The same with the run's conditional group: prefix row G and is_cond.
template <class Acc>
CC_HD inline void cc_focal_walk(const CcShared& sh, const CcTree& t, int f, Acc& acc) {
  if (sh.cond_empty) {
    cc_focal_walk_cond(sh, t, f, nullptr, 0, acc);
    return;
  }
  cc_focal_walk_cond(sh, t, f, t.prefix + sh.G * (sh.N + 1), sh.is_cond[f] ? 1 : 0, acc);
}

}  // namespace colate_cc
