"""Shared by the CondCoalRates edge tests (TEST INFRASTRUCTURE): inputs on a dyadic grid, on which the literal model
(condcoal_model.py), the host twin, the single kernel and the pairs kernel must agree in every bit; the case table of the
CPU matrix with the model's sums and event counters, computed once; and Python restatements of three launch rules of the
device walkers (unit packing, the slab grid, the pieces of a chunk), used only to assert that a case has the layout it is
meant to have.

Why the sums are exact.  Every node height, sample age, epoch and focal epoch of an input is a multiple of Q = 2^-2, and
every tree weight is an integer.  With H the largest height and W the largest |weight|, assert_exact demands

    (1)  H / Q * W < 2^24.

  * A float32 holds every multiple of Q up to 2^24 Q, so `coord` (a float that adds double branch lengths) is the node's
    height exactly, and so are coal_age, lower_age and every epoch that is read (an epoch above H is only compared).
  * a - b, for two such values with a >= b, is a multiple k Q of Q with k <= H / Q: exact.  factor * (a - b) is (W' k) Q with
    an integer |W' k| < 2^24 by (1): exact in float32.  So every addend of denom is an integer multiple of Q, and every
    addend of num an integer.
  * The walk multiplies an addend by a class weight m and a group count (both <= N): an integer below 2^24 N^2 times Q, exact
    in double for every N the library supports.
  * A member x of a sibling subtree adds, for one (focal, conditional) pair and tree, pieces of [lower, coord) that sum to
    |factor| (coord - lower) <= |factor| H, and each of the N haplotypes is such a member at most once on the way up.  So the
    sum of the absolute values of everything a run adds into denom is at most sum_t |factor_t| * F * max(C, 1) * N * H, and
    assert_exact also demands

    (2)  sum_t |factor_t| * F * max(C, 1) * N * H / Q < 2^53.

    Every partial sum, of any subset in any order, is then an integer multiple of Q below 2^53 Q: exact in double.  num's
    addends are smaller (H / Q >= 1).
So the order of summation cannot change a bit: a difference between two implementations is a wrong, missing or extra addend."""
import functools

import numpy as np

import condcoal_model as cm

Q = 0.25
EPOCHS = np.array([0, 8, 16, 32, 64, 128, 256], dtype=np.float32)
EFOCALS = {1: np.array([0], dtype=np.float32), 2: np.array([0, 32], dtype=np.float32),
           3: np.array([0, 16, 64], dtype=np.float32)}
EPOCHS31 = np.array([0.0] + [2.0 ** k for k in range(30)], dtype=np.float32)  # 0, 1, 2, 4, ...: the default grid's size
WEIGHTS = (1.0, 2.0, 3.0, 64.0, 255.0)
KBLOCK = 256       # condcoal_device.hpp: kBlock
KMAXGRID = 1024    # kMaxGrid
KMAXCLOSES = 4     # condcoal_pairs_kernel.hip: kMaxCloses


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def max_height(inp):
    """The largest node height: the root's, of the tallest tree (a node is at least as high as its children)."""
    N = (inp["parents"].shape[1] + 1) // 2
    top = 0.0
    for parent, bl in zip(inp["parents"], inp["branch_lengths"]):
        v, h = 0, 0.0 if inp["sample_ages"] is None else float(inp["sample_ages"][0])
        while parent[v] >= 0:
            h += float(bl[v])
            v = parent[v]
        assert v == 2 * N - 2
        top = max(top, h)
    return top


def assert_exact(inp, epochs, efocal, F=None, C=None):
    """The two conditions of the module docstring, and that everything is on the grid.  F, C: the largest focal and
    conditional list the input is run with (default: its own)."""
    for a in (inp["branch_lengths"], epochs, efocal) + (() if inp["sample_ages"] is None else (inp["sample_ages"],)):
        a = np.asarray(a, dtype=np.float64)
        assert (a >= 0).all() and (a / Q == np.round(a / Q)).all()
    w = np.asarray(inp["factors"], dtype=np.float64)
    assert (w == np.round(w)).all()
    N = (inp["parents"].shape[1] + 1) // 2
    F = len(inp["focal"]) if F is None else F
    C = len(inp["cond"]) if C is None else C
    H = max_height(inp)
    assert H / Q * np.abs(w).max() < 2 ** 24, (H, np.abs(w).max())
    assert np.abs(w).sum() * F * max(C, 1) * N * (H / Q) < 2 ** 53, (np.abs(w).sum(), F, C, N, H)


def dyadic_input(seed, N, T, G, ancient, epochs=EPOCHS, efocal=EFOCALS[2], group_sizes=None, caterpillar_at=None,
                 shuffled_at=None, num_blocks=2, blocks=None, top=300.0):
    """Trees, weights, blocks and groups for colate_amd.condcoal_accumulate, all on the grid of the module docstring.
    A merge is as high as its older child plus zero (a tie), plus the step onto the next epoch or focal boundary above, or
    plus a random multiple of Q (about top / N, so that a caterpillar stays in the low thousands).  Ancient: a third of the
    haplotypes have an age up to 100, half of them on a boundary; nothing lifts the internal nodes above them.
    group_sizes: the exact size of every group (default: random, every group with a member); focal: group 0, cond: group
    1 % G.  caterpillar_at / shuffled_at: the tree that is a caterpillar / whose internal labels are out of coalescence order
    (the root stays 2N-2)."""
    rng = np.random.default_rng(seed)
    bounds = np.unique(np.concatenate([np.asarray(epochs, dtype=np.float64), np.asarray(efocal, dtype=np.float64)]))
    bounds = bounds[(bounds > 0) & (bounds <= 4 * top)]  # (a finer grid's far boundaries would lift the heights off (1))
    nn = 2 * N - 1
    ages = None
    if ancient:
        ages = np.zeros(N)
        idx = rng.choice(N, size=max(1, N // 3), replace=False)
        on = bounds[bounds <= 100.0]
        ages[idx] = np.where(rng.random(idx.size) < 0.5, rng.choice(on, idx.size), Q * rng.integers(1, 400, idx.size))
    span = max(2, int(4 * top / N / Q))
    parents = np.full((T, nn), -1, dtype=np.int32)
    bls = np.zeros((T, nn))
    for t in range(T):
        h = np.zeros(nn)
        if ancient:
            h[:N] = ages
        active = [int(x) for x in rng.permutation(N)]
        for label in range(N, nn):
            # (a caterpillar: the node made last merges again)
            i = len(active) - 1 if (t == caterpillar_at and label > N) else int(rng.integers(len(active)))
            a = active.pop(i)
            b = active.pop(int(rng.integers(len(active))))
            base = max(h[a], h[b])
            r = rng.random()
            if r < 0.25:
                inc = 0.0
            elif r < 0.5:
                above = bounds[bounds > base]
                inc = above.min() - base if above.size else Q
            else:
                inc = Q * int(rng.integers(1, span))
            h[label] = base + inc
            parents[t, a] = parents[t, b] = label
            active.append(label)
        m = parents[t] >= 0
        bls[t, m] = h[parents[t][m]] - h[m]
        if t == shuffled_at and N > 2:
            perm = np.arange(nn)
            perm[N:nn - 1] = rng.permutation(np.arange(N, nn - 1))
            newp = np.full(nn, -1, dtype=np.int32)
            newb = np.zeros(nn)
            for v in range(nn):
                newb[perm[v]] = bls[t, v]
                if parents[t, v] >= 0:
                    newp[perm[v]] = perm[parents[t, v]]
            parents[t], bls[t] = newp, newb
    factors = rng.choice(WEIGHTS, size=T).astype(np.float32)
    factors[-1] = -1.0
    if blocks is None:
        blocks = np.sort(rng.integers(0, num_blocks, size=T))
    blocks = np.asarray(blocks, dtype=np.int32)
    assert blocks.size == T and blocks.min() >= 0 and blocks.max() < num_blocks
    if group_sizes is None:
        group = rng.integers(0, G, size=N).astype(np.int32)
        group[:G] = np.arange(G)
    else:
        assert len(group_sizes) == G and sum(group_sizes) == N and min(group_sizes) >= 1
        group = rng.permutation(np.repeat(np.arange(G), group_sizes)).astype(np.int32)
    inp = dict(parents=parents, branch_lengths=bls, factors=factors, blocks=blocks, num_blocks=num_blocks,
               group_of_hap=group, num_groups=G, focal=np.flatnonzero(group == 0).astype(np.int32),
               cond=np.flatnonzero(group == 1 % G).astype(np.int32), sample_ages=ages)
    sizes = np.bincount(group, minlength=G)
    assert_exact(inp, epochs, efocal, F=int(sizes.max()), C=int(sizes.max()))
    return inp


def model_accumulate(inp, epochs, efocal, events=None, trees=None):
    """The literal model over an input's trees (or its first `trees`): num, denom [num_blocks, EF, E, G]."""
    G = inp["num_groups"]
    num = np.zeros((inp["num_blocks"], len(efocal), len(epochs), G))
    den = np.zeros_like(num)
    for t in range(len(inp["parents"]) if trees is None else trees):
        a, b = cm.tree_accumulators(inp["parents"][t], inp["branch_lengths"][t], inp["factors"][t], inp["group_of_hap"], G,
                                    inp["focal"], inp["cond"], epochs, efocal, inp["sample_ages"], events=events)
        num[inp["blocks"][t]] += a
        den[inp["blocks"][t]] += b
    return num, den


def with_cond(inp, kind):
    """kind: plain (cond = group 1 % G), empty (no conditional haplotype), same (cond = focal)."""
    out = dict(inp)
    if kind == "empty":
        out["cond"] = np.zeros(0, dtype=np.int32)
    elif kind == "same":
        out["cond"] = inp["focal"]
    else:
        assert kind == "plain"
    return out


# ------------------------------------------------------------------ the CPU matrix
CPU_SHAPES = ((2, 1), (3, 2), (24, 4), (40, 9))
CPU_TREES = 5
CPU_CASES = [(ancient, EF, kind, N, G) for ancient in (False, True) for EF in (1, 2, 3)
             for kind in ("plain", "empty", "same") for N, G in CPU_SHAPES]


def cpu_case_id(case):
    ancient, EF, kind, N, G = case
    return f"{'ancient' if ancient else 'modern'}-EF{EF}-{kind}-N{N}-G{G}"


def cpu_input(case):
    ancient, EF, kind, N, G = case
    inp = dyadic_input(7 * N + EF, N, CPU_TREES, G, ancient, efocal=EFOCALS[EF], caterpillar_at=1, shuffled_at=2)
    return with_cond(inp, kind), EPOCHS, EFOCALS[EF]


@functools.lru_cache(maxsize=None)
def cpu_model(case):
    """(num, denom, events) of the literal model on a case of the matrix: computed once, read by every test."""
    inp, epochs, efocal = cpu_input(case)
    events = {}
    num, den = model_accumulate(inp, epochs, efocal, events)
    num.setflags(write=False)
    den.setflags(write=False)
    return num, den, events


# What the CPU matrix as a whole must exercise (counted by the literal model where it happens, each > 0).
COVERAGE = (
    "coord_on_epoch_boundary",                       # a step's coord equal to an epoch boundary
    "coal_age_on_epoch_boundary",
    "modern_coal_age_on_focal_boundary",             # the `<=` search of the class's focal epoch
    "ancient_coal_age_on_focal_boundary",            # the `<` search
    "zero_branch_on_used_step",
    "ancient_lower_advances_s_nonempty_cond",        # lower > coal_age with conditional haplotypes: s searched again ...
    "ancient_lower_advances_ep_nonempty_cond",       # ... and ep
    "ancient_lower_on_focal_boundary",
    "ancient_lower_on_epoch_boundary",
    "focal_search_hits_EF",
    "epoch_search_hits_E",
    "epoch_past_the_end_read_as_inf",
    "class_weight_above_one",
    "modern_sibling_smaller_than_G",                 # the by-member path of the modern walk
    "modern_sibling_at_least_G",                     # the by-group path
)


def cpu_coverage():
    total = {}
    for case in CPU_CASES:
        for k, v in cpu_model(case)[2].items():
            total[k] = total.get(k, 0) + v
    return total


# ------------------------------------------------------------------ launch rules of the device walkers, restated
def unit_start(pair_sizes):
    """condcoal_pairs_kernel.hip, PairsWalker::init: consecutive pairs are packed into units of at most KBLOCK items; a
    pair with more is a unit of its own.  Returns (pair_start, unit_start)."""
    pair_start, units = [0], [0]
    for p, n in enumerate(pair_sizes):
        pair_start.append(pair_start[-1] + n)
        if pair_start[p + 1] - units[-1] > KBLOCK and pair_start[p] > units[-1]:
            units.append(pair_start[p])
    units.append(pair_start[-1])
    return pair_start, units


def unit_layout(pair_sizes):
    """What a pair list's units offer: (a unit of exactly KBLOCK items made of two pairs or more, a unit above KBLOCK, a
    batch of a unit inside which one pair ends and the next begins)."""
    pair_start, units = unit_start(pair_sizes)
    full = above = seam = False
    for u0, u1 in zip(units[:-1], units[1:]):
        inside = [s for s in pair_start if u0 < s < u1]
        full |= (u1 - u0 == KBLOCK and len(inside) >= 1)
        above |= u1 - u0 > KBLOCK
        for b in range(u0, u1, KBLOCK):
            seam |= any(b < s < min(b + KBLOCK, u1) for s in inside)
    return full, above, seam


# P1 of the GPU cases: group sizes and (focal group, conditional group) pairs whose focal lists are, in order,
# 3 253 | 300 | 1 | 256 | 257 | 2 | 300 | 3 haplotypes (| : a unit's end)
P1_SIZES = (3, 253, 300, 1, 256, 257, 2)
P1_PAIRS = ([0, 1, 2, 3, 4, 5, 6, 2, 0], [1, 0, 3, -1, 4, 2, 6, -1, 0])


def p1_input(ancient):
    inp = dyadic_input(61 + ancient, sum(P1_SIZES), 4, len(P1_SIZES), ancient, efocal=EFOCALS[3], group_sizes=P1_SIZES,
                       caterpillar_at=1)
    assert unit_layout([P1_SIZES[f] for f in P1_PAIRS[0]]) == (True, True, True)
    return inp


def slab_grid(work, S):
    """condcoal_device.hpp: the workgroups of a walk kernel, whose slabs take KBLOCK * S doubles each and 2 GiB at most."""
    return max(1, min(KMAXGRID, work, (2 << 30) // (KBLOCK * S * 8)))


def launch_pieces(blocks):
    """PairsWalker::submit on the first chunk of a run: the pieces a chunk with these blocks is launched in, each of which
    closes at most KMAXCLOSES blocks.  Returns the number of trees of each piece."""
    pieces, t0, closes, cur = [], 0, 0, -1
    for t, b in enumerate(blocks):
        if b != cur:
            if cur >= 0 and closes == KMAXCLOSES:
                pieces.append(t - t0)
                t0, closes = t, 0
            closes += cur >= 0
            cur = b
    pieces.append(len(blocks) - t0)
    return pieces
