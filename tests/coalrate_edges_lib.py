"""Shared by the CoalRate edge tests (TEST INFRASTRUCTURE): a library of constructed cases for the two device paths of
`CoalRate` (coalrate_kernel.hip: cr_count / cr_fold; coalrate_tree_kernel.hip: crt_sort / crt_fold).  Every case is built
deterministically from its name, carries the launch shape it is meant to take (`expect`: what colate_amd.coalrate_launch_shape
/ coalrate_tree_launch_shape must report after the device call) and a self-check that proves, on the CPU, that the case is
what its name says.  The Python restatements of the walkers' sizing rules below (lanes per call, LDS bytes, stretch lengths)
serve those self-checks only; which path a call took on the device is what the getters say.

Models.  `pairwise`: coalrate_model.Model, the literal pair-by-pair restatement.  `exact` (la_exact): trees with integer node
times under integer epochs, modern samples and weights that are multiples of 1e9 -- every addend is then an integer below
2^53, so every order of summation gives the same bits and the host twin must equal the model exactly.  `tree`:
coalrate_tree_model.accumulate.  `hand`: the sums written out in the case.

Child runs (`python coalrate_edges_lib.py MODE NAME OUT.npz DEVICE`): the child builds the case again from its name, runs
it (DEVICE 1: the device call, 0: the host twin; NAME `all` with DEVICE 0: the twin of every case of the mode) and saves
num, den and the getter's values.  `python coalrate_edges_lib.py refusals - OUT.npz 1`: the two refusals of the device walkers,
each followed by an accepted call."""
import functools
import os
import subprocess
import sys

import numpy as np

import coalrate_lib as cl
import coalrate_tree_lib as tl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

K_MAX_LANES = 256          # coalrate_device.hpp kMaxLanes
K_LDS_BYTES = 160 * 1024   # kLdsBytes
K_WAVES_PER_CU = 8         # kWavesPerCu
K_PARTIALS = 64            # coalrate_tree.h kPartials
K_LDS_KEYS = 16384         # kLdsKeys
K_MAX_EPOCHS = 1024        # kMaxDeviceEpochs
K_MAX_N = 16384            # kMaxHaplotypes
MI355X_CUS = 256           # the chip the packed cases are sized for
SHAPE_KEYS = cl.SHAPE_KEYS

LA_EPOCHS = cl.bins_epochs(2.0, 6.0, 0.25)
INT_EPOCHS = np.array([0.0, 1.0, 3.0, 7.0, 100.0, 1000.0, 5000.0, 20000.0, 1e6])   # for the exact model
SMALL_EPOCHS = np.array([0.0, 10.0, 100.0, 1000.0, 1e5])
TIE6 = np.array([0.0, 64.0, 128.0, 1024.0, 4096.0, 1e7])   # tl.TIE_EPOCHS with one more: E - 1 = 5 is odd
G_OF_LPC = {1: 1, 4: 2, 8: 3, 16: 4, 32: 6, 64: 8, 128: 11, 256: 16}
TREE_LPC_N = (2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ the walkers' sizing rules, for the self-checks
def la_lpc(G):
    """Lanes per call of cr_count: the power of two that holds the group pairs, at most 256."""
    lpc = 1
    while lpc < G * (G + 1) // 2 and lpc < K_MAX_LANES:
        lpc *= 2
    return lpc


def la_lds_bytes(N, G):
    """(labels and per-lane counts, prefix rows) of one call, in bytes."""
    return 2 * (N + la_lpc(G) * G), 2 * G * (N + 1)


def tree_lpc(N):
    return min(K_MAX_LANES, max(4, tl.padded_keys(N) // 2))


def tree_stretch(N):
    """Positions per lane of crt_sort's scan: ceil(nn / lpc) | 1."""
    return (-(-(2 * N - 1) // tree_lpc(N))) | 1


def packed_cpw(calls, lpc, cus):
    """Calls per workgroup of a chunk of `calls` calls on a chip of `cus` CUs, where the LDS does not bind."""
    waves = (lpc + 63) // 64
    return max(1, min(K_MAX_LANES // lpc, -(-calls * waves // (cus * K_WAVES_PER_CU))))


def shape(launches, cpw, lpc, lds, cpw_min=None):
    return dict(launches=launches, cpw_min=cpw if cpw_min is None else cpw_min, cpw_max=cpw, lanes_per_call=lpc, lds=int(lds))


# ------------------------------------------------------------------ constructed trees (numpy; Relate labelling, root 2N-2)
def from_heights(parent, h):
    return parent, np.where(parent >= 0, h[np.maximum(parent, 0)] - h, 0.0)


def caterpillar(N, heights, order=None, ages=None):
    """Internal node N + j joins leaf order[j + 1] to everything below it, at heights[j] (non-decreasing)."""
    nn = 2 * N - 1
    order = np.arange(N) if order is None else np.asarray(order)
    heights = np.asarray(heights, dtype=float)
    assert heights.shape == (N - 1,) and (np.diff(heights) >= 0).all()
    parent = np.full(nn, -1, dtype=np.int32)
    parent[order[0]] = N
    parent[order[1:]] = N + np.arange(N - 1)
    parent[N:nn - 1] = np.arange(N + 1, nn)
    h = np.zeros(nn)
    if ages is not None:
        h[:N] = ages
    h[N:] = heights
    return from_heights(parent, h)


def balanced(N, level_height=1.0, order=None):
    """The node over leaf positions [a, b) splits at (a + b) // 2; it lies at level_height * ceil(log2(b - a)), so that all
    nodes of a level tie.  Labels ascend with the size of the range: a child's label is below its parent's."""
    nn = 2 * N - 1
    order = np.arange(N) if order is None else np.asarray(order)
    ranges, stack = [], [(0, N)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        ranges.append((a, b))
        m = (a + b) // 2
        stack += [(a, m), (m, b)]
    ranges.sort(key=lambda r: (r[1] - r[0], r[0]))
    label = {r: N + i for i, r in enumerate(ranges)}
    parent = np.full(nn, -1, dtype=np.int32)
    h = np.zeros(nn)
    for (a, b), v in label.items():
        m = (a + b) // 2
        for c in ((a, m), (m, b)):
            parent[order[c[0]] if c[1] - c[0] == 1 else label[c]] = v
        h[v] = level_height * (b - a - 1).bit_length()
    assert label[(0, N)] == nn - 1
    return from_heights(parent, h)


def heights_of(parent, bl, ages=None):
    """Node heights in double from the branch lengths; needs child labels below parent labels (the trees built here)."""
    nn = len(parent)
    N = (nn + 1) // 2
    h = np.zeros(nn)
    if ages is not None:
        h[:N] = ages
    for v in range(nn - 1):
        assert parent[v] > v
        h[parent[v]] = max(h[parent[v]], h[v] + bl[v])
    return h


def node_epoch(epochs, t):
    """The cell of a node at time t: epochs[e] < t <= epochs[e + 1] (cell 0 from t = 0)."""
    return np.maximum(0, np.searchsorted(np.asarray(epochs)[1:], t, side="left"))


# ------------------------------------------------------------------ the exact model of local_ancestry
def la_exact(case):
    """num / den [blocks][G][G][E] in exact integers, from pair semantics: a pair of leaves that meets at node v (time t, cell
    e_v) adds w / 1e9 to num[e_v], width[e] * w / 1e9 to den[e] for every e < e_v and (t - epochs[e_v]) * w / 1e9 to
    den[e_v].  Per node and group pair the number of such pairs comes from the children's per-group leaf counts."""
    epochs, G = case["epochs"], case["G"]
    assert case["ages"] is None and (epochs == np.round(epochs)).all()
    E = len(epochs)
    width = np.append(np.diff(epochs), 0.0).astype(np.int64)
    num = np.zeros((case["num_blocks"], G, G, E), dtype=np.int64)
    den = np.zeros_like(num)
    for k in range(len(case["weights"])):
        parent, w = case["parents"][k], case["weights"][k] / 1e9
        assert w == round(w)
        nn = len(parent)
        N = (nn + 1) // 2
        h = heights_of(parent, case["bl"][k])
        assert (h == np.round(h)).all()
        kids = np.argsort(parent[:-1], kind="stable")
        c0, c1 = kids[0::2], kids[1::2]
        assert (parent[c0] == N + np.arange(N - 1)).all() and (parent[c1] == parent[c0]).all()
        cnt = np.zeros((nn, G), dtype=np.int64)
        cnt[np.arange(N), case["groups"][case["gv"][k]]] = 1
        for j in range(N - 1):
            cnt[N + j] = cnt[c0[j]] + cnt[c1[j]]
        L, R = cnt[c0], cnt[c1]
        m = L[:, :, None] * R[:, None, :] + L[:, None, :] * R[:, :, None]      # [node][g1][g2], g1 != g2
        m[:, np.arange(G), np.arange(G)] //= 2
        m *= np.tril(np.ones((G, G), dtype=np.int64))                         # filled for g1 >= g2 only
        t = h[N:].astype(np.int64)
        ev = node_epoch(epochs, h[N:])
        b = case["blocks"][k]
        for e in range(E):
            here, later = ev == e, ev > e
            num[b, :, :, e] += int(w) * m[here].sum(axis=0)
            den[b, :, :, e] += int(w) * (width[e] * m[later].sum(axis=0) + (m[here] * (t[here] - int(epochs[e]))[:, None, None]).sum(axis=0))
    assert max(np.abs(num).max(), np.abs(den).max()) < 2 ** 53
    return num.astype(np.float64), den.astype(np.float64)


# ------------------------------------------------------------------ local_ancestry cases
def _la_case(parents, bl, weights, blocks, num_blocks, gv, groups, G, epochs, ages, expect, check, model, chunk=None, distinct=None,
             hand=None, packed=False):
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    return dict(mode="la", parents=parents, bl=np.asarray(bl, dtype=float), weights=np.asarray(weights, dtype=float),
                blocks=np.asarray(blocks, dtype=np.int32), num_blocks=num_blocks, gv=np.asarray(gv, dtype=np.int32),
                groups=np.ascontiguousarray(groups, dtype=np.int32), G=G, epochs=np.asarray(epochs, dtype=float), ages=ages,
                expect=expect, check=check, model=model, chunk=chunk, distinct=distinct, hand=hand, packed=packed)


def _stack(trees):
    return np.array([t[0] for t in trees]), np.array([t[1] for t in trees])


def _la_lpc(lpc):
    G = G_OF_LPC[lpc]
    N, T = 13, 6
    rng = np.random.default_rng(4000 + G)
    ages = np.zeros(N)
    ages[[1, 4, 7, 10]] = [5.0, 8.0, 30.0, 5.0]
    parents, bl = _stack([cl.random_tree(rng, N, ages) for _ in range(T)])
    groups = (np.arange(N)[None, :] * np.array([1, 3, 5])[:, None] + np.array([0, 1, 2])[:, None]) % G

    def check(c):
        assert la_lpc(G) == lpc and (lpc == 1 or N % lpc != 0)
        assert len({int(node_epoch(c["epochs"], a)) for a in ages if a > 0}) >= 2      # ancient samples in two age epochs
        assert len(set(c["gv"].tolist())) == 3 and sum(la_lds_bytes(N, G)) <= K_LDS_BYTES
    return _la_case(parents, bl, [1500.5, 20.25, 8999.0, 0.5, 333.125, 4100.0], [0, 0, 1, 1, 1, 2], 3, [0, 1, 2, 0, 1, 2], groups, G,
                    LA_EPOCHS, ages, shape(1, 1, lpc, True), check, "pairwise")


def _la_packed(name):
    G, N, T, epochs, intended = {"packed_two_waves": (11, 4, 1100, LA_EPOCHS, 2),
                                 "packed_cap": (8, 4, 6200, np.array([0.0, 300.0, 1e7]), 4)}[name]
    D = 10
    rng = np.random.default_rng(4100 + G)
    parents, bl = _stack([cl.random_tree(rng, N, Ne=200.0) for _ in range(D)])
    weights = 1.0 + 0.5 * np.arange(T)
    if name == "packed_cap":
        weights[100] = 0.0      # a tree of weight 0 makes no call: 6199 calls, the last workgroup holds three
    calls = int((weights != 0).sum())
    groups = np.array([[0, 5, 10, 5], [10, 10, 3, 0], [1, 2, 3, 4]]) % G
    lpc = la_lpc(G)

    def check(c):
        assert lpc == {"packed_two_waves": 128, "packed_cap": 64}[name]
        assert packed_cpw(calls, lpc, MI355X_CUS) == intended == K_MAX_LANES // lpc       # the lane cap: cpw * lpc == kMaxLanes
        assert calls * ((lpc + 63) // 64) > (intended - 1) * MI355X_CUS * K_WAVES_PER_CU
        assert intended * sum(la_lds_bytes(N, G)) <= K_LDS_BYTES                          # the LDS does not bind
        assert len(np.unique(weights)) == T
        if name == "packed_cap":
            assert calls % intended != 0 and len(c["epochs"]) == 3
    return _la_case(np.tile(parents, (T // D, 1)), np.tile(bl, (T // D, 1)), weights, np.arange(T) * 4 // T, 4, np.arange(T) % 3, groups,
                    G, epochs, None, shape(1, intended, lpc, True), check, "pairwise", distinct=D, packed=True)


def _int_trees(N, seed):
    """Two trees with integer node times: a caterpillar over a shuffled leaf order (times 1 .. N-1) and the balanced tree
    (times = levels)."""
    order = np.random.default_rng(seed).permutation(N)
    return [caterpillar(N, 1.0 + np.arange(N - 1), order), balanced(N)]


def _la_lds(name):
    N, G = {"lds_last": 2786, "lds_first": 2787}[name], 26
    parents, bl = _stack(_int_trees(N, 4200))
    groups = np.array([np.arange(N) % G, np.arange(N) // 108 % G])
    fits = name == "lds_last"

    def check(c):
        assert (sum(la_lds_bytes(N, G)) <= K_LDS_BYTES) == fits
        assert sum(la_lds_bytes(2786, G)) <= K_LDS_BYTES < sum(la_lds_bytes(2787, G)) and la_lpc(G) == 256
    return _la_case(parents, bl, [1e9, 2e9], [1, 0], 2, [0, 1], groups, G, INT_EPOCHS, None, shape(1, 1, 256, fits), check, "exact")


def _la_max_N(G):
    N = K_MAX_N
    trees = _int_trees(N, 4300)
    parents, bl = _stack([trees[0], trees[1]] if G == 1 else [trees[0], trees[0], trees[1], trees[1]])
    groups = np.zeros((1, N)) if G == 1 else np.array([np.zeros(N), np.arange(N) // 3 % 2])
    T = len(parents)

    def check(c):
        assert N == 16384 and (c["groups"][0] == 0).all()              # every leaf in group 0
        assert heights_of(c["parents"][0], c["bl"][0]).max() == N - 1
        assert sum(la_lds_bytes(N, G)) <= K_LDS_BYTES
    return _la_case(parents, bl, 1e9 * (1 + np.arange(T)), np.arange(T) % 2, 2, np.arange(T) % G, groups, G, INT_EPOCHS, None, shape(1, 1, la_lpc(G), True), check, "exact")


def _la_max_G():
    N, G = 8, 319
    rng = np.random.default_rng(4400)
    parents, bl = _stack([cl.random_tree(rng, N) for _ in range(3)])
    groups = np.array([[0, 318, 5, 5, 100, 318, 0, 7], [318, 317, 316, 1, 2, 3, 4, 0]])

    def check(c):
        assert la_lds_bytes(N, G)[0] <= K_LDS_BYTES < la_lds_bytes(N, G + 1)[0]       # G + 1 is refused
        assert sum(la_lds_bytes(N, G)) > K_LDS_BYTES and len(c["epochs"]) == 2
    return _la_case(parents, bl, [700.5, 1.25, 42.0], [0, 1, 1], 2, [0, 1, 0], groups, G, [0.0, 1e7], None, shape(1, 1, 256, False),
                    check, "pairwise")


def _la_small(name):
    N, G = 8, 3
    rng = np.random.default_rng(4500)
    lpc = la_lpc(G)
    if name in ("empty_group", "one_group"):
        trees = _int_trees(N, 4501) + _int_trees(N, 4502)
        parents, bl = _stack(trees)
        groups = np.array([[0, 2, 2, 0, 0, 2, 0, 2], [2, 2, 0, 2, 2, 0, 0, 0]] if name == "empty_group" else [[2] * N, [0] * N])

        def check(c):
            if name == "empty_group":
                assert not (c["groups"] == 1).any() and set(np.unique(c["groups"])) == {0, 2}
            else:
                assert all(len(set(v.tolist())) == 1 for v in c["groups"])
        return _la_case(parents, bl, [1e9, 3e9, 2e9, 5e9], [0, 0, 1, 1], 2, [0, 1, 1, 0], groups, G, INT_EPOCHS, None,
                        shape(1, 1, lpc, True), check, "exact")
    groups = rng.integers(0, G, (2, N))
    if name == "returning_blocks":
        parents, bl = _stack([cl.random_tree(rng, N) for _ in range(6)])
        blocks = [0, 1, 0, 2, 1, 0]

        def check(c):
            b = c["blocks"].tolist()
            assert b == blocks and c["chunk"] is None
            assert any(b[i] in b[:i - 1] and b[i - 1] != b[i] for i in range(2, len(b)))      # a block comes back after another
        return _la_case(parents, bl, [10.5, 200.0, 3.25, 47.0, 1000.0, 8.0], blocks, 3, [0, 1, 1, 0, 0, 1], groups, G, LA_EPOCHS, None,
                        shape(1, 1, lpc, True), check, "pairwise")
    if name == "all_zero_weight_chunk":
        parents, bl = _stack([cl.random_tree(rng, N) for _ in range(8)])

        def check(c):
            assert c["chunk"] == 4 and (c["weights"][:4] != 0).all() and (c["weights"][4:] == 0).all()
        return _la_case(parents, bl, [10.5, 200.0, 3.25, 47.0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1, 2, 2], 3, [0, 1, 1, 0, 0, 1, 0, 1], groups,
                        G, LA_EPOCHS, None, shape(1, 1, lpc, True), check, "pairwise", chunk=4)
    if name == "all_in_last_epoch":
        parents, bl = _stack([caterpillar(N, 200.0 + 100.0 * np.arange(N - 1), rng.permutation(N)), balanced(N, 250.0)])
        epochs = SMALL_EPOCHS[:4]

        def check(c):
            for p, b in zip(c["parents"], c["bl"]):
                assert (node_epoch(epochs, heights_of(p, b)[N:]) == len(epochs) - 2).all()
        return _la_case(parents, bl, [10.5, 200.0], [0, 0], 1, [0, 1], groups, G, epochs, None, shape(1, 1, lpc, True), check, "pairwise")
    assert name == "smallest"
    # N = 2: one node; (time, weight, group vector, block) per call under epochs 0, 10, 100, 1000
    parents = np.array([[2, 2, -1]] * 3)
    bl = np.array([[5.0, 5.0, 0.0], [50.0, 50.0, 0.0], [100.0, 100.0, 0.0]])
    epochs = SMALL_EPOCHS[:4]
    num = np.zeros((2, G, G, 4))
    den = np.zeros((2, G, G, 4))
    num[0, 2, 0, 0], den[0, 2, 0, 0] = 1.0, 5.0                                       # the pair (0, 2) meets at 5 in cell 0
    num[0, 1, 1, 1], den[0, 1, 1, 0], den[0, 1, 1, 1] = 2.0, 2 * 10.0, 2 * 40.0       # (1, 1) at 50: all of cell 0, 40 of cell 1
    num[1, 2, 0, 1], den[1, 2, 0, 0], den[1, 2, 0, 1] = 3.0, 3 * 10.0, 3 * 90.0       # (0, 2) at 100, on the boundary: cell 1

    def check(c):
        assert c["parents"].shape == (3, 3)
    return _la_case(parents, bl, [1e9, 2e9, 3e9], [0, 0, 1], 2, [0, 1, 0], [[0, 2], [1, 1]], G, epochs, None, shape(1, 1, lpc, True),
                    check, "pairwise", hand=(num, den))


LA_BUILDERS = {f"lpc_{k}": functools.partial(_la_lpc, k) for k in G_OF_LPC}
LA_BUILDERS.update({n: functools.partial(_la_packed, n) for n in ("packed_two_waves", "packed_cap")})
LA_BUILDERS.update({n: functools.partial(_la_lds, n) for n in ("lds_last", "lds_first")})
LA_BUILDERS.update({"max_N_G1": functools.partial(_la_max_N, 1), "max_N_G2": functools.partial(_la_max_N, 2), "max_G": _la_max_G})
LA_BUILDERS.update({n: functools.partial(_la_small, n) for n in ("empty_group", "one_group", "returning_blocks", "all_zero_weight_chunk",
                                                                   "smallest", "all_in_last_epoch")})


# ------------------------------------------------------------------ tree cases
def _tree_case(parents, bl, weights, blocks, num_blocks, epochs, ages, expect, check, chunk=None, distinct=None, hand=None, packed=False):
    return dict(mode="tree", parents=np.ascontiguousarray(parents, dtype=np.int32), bl=np.asarray(bl, dtype=float),
                weights=np.asarray(weights, dtype=float), blocks=np.asarray(blocks, dtype=np.int32), num_blocks=num_blocks,
                epochs=np.asarray(epochs, dtype=float), ages=ages, expect=expect, check=check, model="tree", chunk=chunk,
                distinct=distinct, hand=hand, packed=packed)


def sorted_times(c, k):
    """The float32 node times of call k in the sort's order, and the labels in that order."""
    import coalrate_tree_model as tm
    t = tm.node_times(c["parents"][k], c["bl"][k], c["ages"])
    order = np.lexsort((np.arange(len(t)), t))
    return t[order], order


def last_tie_group_stretches(c, k):
    """How many lane stretches of crt_sort's scan the tie group that ends at the last position covers."""
    st, _ = sorted_times(c, k)
    N = (len(st) + 1) // 2
    first = int(np.searchsorted(st, st[-1], side="left"))
    return (len(st) - 1) // tree_stretch(N) - first // tree_stretch(N) + 1, len(st) - first


def _tree_lpc(N):
    rng = np.random.default_rng(5000 + N)
    parents, bl, weights, blocks, ages = tl.random_input(rng, N, 6, 2, True, TIE6, 64.0)
    if N == 2:
        # quantised_tree puts the root at the ancient sample's age, where two lineages never coexist (denom 0): every other
        # tree gets its root one quantum later
        bl[::2, :2] += 64.0
    lpc = tree_lpc(N)

    def check(c):
        per = max(1, lpc // K_PARTIALS)
        assert per == 1 or (len(TIE6) - 1) % per != 0          # the last group of epochs is not full
        assert (ages > 0).any()
        assert N == 2 or tree_lpc(N - 1) < lpc or tree_lpc(N + 1) > lpc          # an end of its class of lanes per call
        sorts = [sorted_times(c, k) for k in range(6)]
        times = np.concatenate([st for st, _ in sorts])
        assert np.isin(TIE6[1:-1], times).sum() >= (2 if N >= 33 else 1)         # node times on epoch boundaries
        assert N == 2 or any(len(np.unique(st[order >= N])) < N - 1 for st, order in sorts)      # ties among internal nodes
    return _tree_case(parents, bl, weights, blocks, 2, TIE6, ages, shape(1, 1, lpc, True), check)


def _tree_packed(name):
    N, T, intended = {"packed_two_waves": (65, 1100, 2), "packed_cap": (33, 6200, 4)}[name]
    D = 10
    rng = np.random.default_rng(5100 + N)
    parents, bl, _, _, ages = tl.random_input(rng, N, D, 1, True, TIE6, 64.0)
    weights = 1.0 + 0.5 * np.arange(T)
    lpc = tree_lpc(N)

    def check(c):
        assert lpc == {"packed_two_waves": 128, "packed_cap": 64}[name]
        assert packed_cpw(T, lpc, MI355X_CUS) == intended == K_MAX_LANES // lpc           # the lane cap: cpw * lpc == kMaxLanes
        assert T * ((lpc + 63) // 64) > (intended - 1) * MI355X_CUS * K_WAVES_PER_CU
        assert len(np.unique(weights)) == T
    return _tree_case(np.tile(parents, (T // D, 1)), np.tile(bl, (T // D, 1)), weights, np.arange(T) * 4 // T, 4, TIE6, ages,
                      shape(1, intended, lpc, True), check, distinct=D, packed=True)


def _tree_max_N():
    N = K_MAX_N
    parents, bl = _stack([caterpillar(N, 1.0 + np.arange(N - 1) // 4), balanced(N, 64.0)])

    def check(c):
        assert tl.padded_keys(N) == 32768 > K_LDS_KEYS
        assert last_tie_group_stretches(c, 0)[1] == 3                 # the caterpillar: ties of four, three at the end
        st, _ = sorted_times(c, 1)
        assert (st == 64.0).sum() == N // 2 and (st == 128.0).sum() == N // 4       # the balanced tree: a level is one tie group
    return _tree_case(parents, bl, [1234.5, 777.25], [0, 1], 2, TIE6, None, shape(1, 1, 256, False), check)


def _tree_E(name):
    N = 40
    if name == "E_2":
        # caterpillars with a node every `step`: L lineages over each step, L = 40 .. 2, so den = wq * step * sum L (L - 1) / 2
        steps, wq, blocks = [64.0, 32.0, 64.0], [1.0, 2.0, 3.0], [0, 0, 1]
        parents, bl = _stack([caterpillar(N, s * (1.0 + np.arange(N - 1))) for s in steps])
        pairs_sum = sum(L * (L - 1) // 2 for L in range(2, N + 1))
        assert pairs_sum == 10660      # C(41, 3)
        num = np.array([[39 * 1.0 + 39 * 2.0, 0.0], [39 * 3.0, 0.0]])
        den = np.array([[64.0 * 10660 * 1.0 + 32.0 * 10660 * 2.0, 0.0], [64.0 * 10660 * 3.0, 0.0]])

        def check(c):
            assert len(c["epochs"]) == 2
        return _tree_case(parents, bl, 1e9 * np.array(wq), blocks, 2, [0.0, 1e7], None, shape(1, 1, tree_lpc(N), True), check,
                          hand=(num, den))
    rng = np.random.default_rng(5200)
    E = K_MAX_EPOCHS + (name == "E_1025")
    epochs = np.append(8.0 * np.arange(E - 1), 1e7)
    parents, bl, weights, blocks, ages = tl.random_input(rng, N, 4, 2, True, epochs, 64.0)

    def check(c):
        assert len(c["epochs"]) == E
        import coalrate_tree_model as tm
        for k in range(4):
            t = tm.node_times(c["parents"][k], c["bl"][k], ages)
            assert t.max() < epochs[-2] and len(np.unique(node_epoch(epochs, t))) < E // 10       # many epochs hold no node
    return _tree_case(parents, bl, weights, blocks, 2, epochs, ages, shape(1, 1, tree_lpc(N), True), check)


def _tree_shaped(name, N):
    import coalrate_tree_model as tm
    rng = np.random.default_rng(5300 + N)
    T, nn, lpc = 4, 2 * N - 1, tree_lpc(N)
    ages = None
    weights, blocks, nb = [1500.5, 20.25, 8999.0, 333.125], [0, 0, 1, 1], 2
    base = [tl.quantised_tree(rng, N) for _ in range(T)]
    hand = None
    if name == "one_tie_group":
        trees = []
        for p, _ in base:
            h = np.zeros(nn)
            h[N:] = 128.0          # (an epoch boundary too)
            trees.append(from_heights(p, h))

        def check(c):
            for k in range(T):
                stretches, members = last_tie_group_stretches(c, k)
                assert members == N - 1 and stretches >= 13
    elif name == "all_at_zero":
        trees = [(p, np.zeros(nn)) for p, _ in base]
        wq = np.array(weights) / 1e9
        num = np.zeros((nb, len(TIE6)))
        num[0, 0] = (0.0 + (N - 1) * wq[0]) + (N - 1) * wq[1]         # N - 1 internal nodes in cell 0, call by call
        num[1, 0] = (0.0 + (N - 1) * wq[2]) + (N - 1) * wq[3]
        hand = (num, np.zeros((nb, len(TIE6))))                        # every piece has length 0

        def check(c):
            assert not c["bl"].any() and last_tie_group_stretches(c, 0)[1] == nn
    elif name == "all_in_last_epoch":
        trees = [caterpillar(N, TIE6[-2] + 64.0 * (1 + np.arange(N - 1) // 2), rng.permutation(N)) for _ in range(T)]

        def check(c):
            for k in range(T):
                st, order = sorted_times(c, k)
                assert (node_epoch(TIE6, st[order >= N]) == len(TIE6) - 2).all() and (st[order < N] == 0).all()
    elif name == "all_ancient":
        ages = 64.0 * (1 + np.arange(N) % 3)
        trees = [tl.quantised_tree(rng, N, ages) for _ in range(T)]

        def check(c):
            assert (c["ages"] > 0).all() and sorted_times(c, 0)[0][0] > 0
    elif name == "tie_to_the_end":
        trees = []
        for p, b in base:
            h = tm.node_times(p, b).astype(float)
            assert (np.diff(h[N:]) >= 0).all()         # labels in time order: the last four are the root and three below it
            h[nn - 4:] = h[nn - 1]
            trees.append(from_heights(p, h))

        def check(c):
            for k in range(T):
                assert last_tie_group_stretches(c, k)[1] >= 4
            assert any(last_tie_group_stretches(c, k)[0] >= 2 for k in range(T))
    else:
        assert name == "returning_blocks"
        trees = base + [tl.quantised_tree(rng, N) for _ in range(2)]
        weights, blocks, nb = weights + [47.0, 8.0], [0, 1, 0, 2, 1, 0], 3

        def check(c):
            assert c["blocks"].tolist() == [0, 1, 0, 2, 1, 0] and c["chunk"] is None
    parents, bl = _stack(trees)
    return _tree_case(parents, bl, weights, blocks, nb, TIE6, ages, shape(1, 1, lpc, True), check, hand=hand)


TREE_SHAPED = ("one_tie_group", "all_at_zero", "all_in_last_epoch", "all_ancient", "tie_to_the_end", "returning_blocks")
TREE_BUILDERS = {f"lpc_{N}": functools.partial(_tree_lpc, N) for N in TREE_LPC_N}
TREE_BUILDERS.update({n: functools.partial(_tree_packed, n) for n in ("packed_two_waves", "packed_cap")})
TREE_BUILDERS.update({"max_N": _tree_max_N, "E_2": functools.partial(_tree_E, "E_2"), "E_1024": functools.partial(_tree_E, "E_1024")})
TREE_BUILDERS.update({f"{n}_{N}": functools.partial(_tree_shaped, n, N) for n in TREE_SHAPED for N in (40, 300)})
BUILDERS = {"la": LA_BUILDERS, "tree": TREE_BUILDERS}


def names(mode):
    return list(BUILDERS[mode])


@functools.lru_cache(maxsize=None)
def case(mode, name):
    return BUILDERS[mode][name]()


def cases(mode):
    """name -> case, every case of the mode built."""
    return {n: case(mode, n) for n in BUILDERS[mode]}


def refused_cases():
    """Inputs the device walkers refuse with COLATE_ELIMIT: G = 320 at N = 8 (the labels and group counts of one tree are
    more than the LDS), and 1025 epochs in tree mode."""
    c = dict(_la_max_G())
    c["G"] = 320
    assert la_lds_bytes(8, 320)[0] > K_LDS_BYTES
    return {"la": c, "tree": _tree_E("E_1025")}


# ------------------------------------------------------------------ running a case
def accumulate(c, device, first=None):
    """The case through colate_amd in this process (first: only its first calls); sets and restores the chunk cap."""
    import colate_amd
    old = os.environ.pop("COLATE_COALRATE_CHUNK_TREES", None)
    if c["chunk"]:
        os.environ["COLATE_COALRATE_CHUNK_TREES"] = str(c["chunk"])
    try:
        s = slice(0, first)
        if c["mode"] == "la":
            return colate_amd.coalrate_accumulate(c["parents"][s], c["bl"][s], c["weights"][s], c["blocks"][s], c["num_blocks"], c["gv"][s],
                                                  c["groups"], c["G"], c["epochs"], c["ages"], device=device)
        return colate_amd.coalrate_tree_accumulate(c["parents"][s], c["bl"][s], c["weights"][s], c["blocks"][s], c["num_blocks"],
                                                   c["epochs"], c["ages"], device=device)
    finally:
        os.environ.pop("COLATE_COALRATE_CHUNK_TREES", None)
        if old is not None:
            os.environ["COLATE_COALRATE_CHUNK_TREES"] = old


def launch_shape(mode):
    import colate_amd
    return colate_amd.coalrate_launch_shape() if mode == "la" else colate_amd.coalrate_tree_launch_shape()


def run_child(tmp_path, mode, name, device, timeout):
    """One child under its own time limit; returns the arrays it saved; raises on a child that fails (nothing is retried)."""
    dst = os.path.join(str(tmp_path), f"edges_{mode}_{name}_{int(device)}.npz")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + HERE + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, name, dst, str(int(device))], capture_output=True, text=True,
                       env=env, timeout=timeout)
    assert r.returncode == 0, (mode, name, r.returncode, r.stderr[-2000:])
    return dict(np.load(dst))


def _refusals():
    import colate_amd
    out = {}
    for mode, c in refused_cases().items():
        try:
            accumulate(c, True)
            out[f"{mode}_code"], out[f"{mode}_message"] = 0, ""
        except colate_amd.ColateError as e:
            out[f"{mode}_code"], out[f"{mode}_message"] = e.code, str(e)
        out[f"{mode}_shape_refused"] = [launch_shape(mode)[k] for k in SHAPE_KEYS]
        ok = case(mode, "max_G" if mode == "la" else "E_1024")        # the nearest accepted input, in the same process
        dnum, dden = accumulate(ok, True)
        out[f"{mode}_shape"] = [launch_shape(mode)[k] for k in SHAPE_KEYS]
        hnum, hden = accumulate(ok, False)
        out[f"{mode}_same"] = same_bits(dnum, hnum) and same_bits(dden, hden) and bool((hnum != 0).any())
    return out


if __name__ == "__main__":
    mode, name, dst, device = sys.argv[1], sys.argv[2], sys.argv[3], bool(int(sys.argv[4]))
    if mode == "refusals":
        np.savez(dst, **_refusals())
    elif name == "all":
        assert not device
        out = {}
        for n in names(mode):
            out[f"num_{n}"], out[f"den_{n}"] = accumulate(case(mode, n), False)
        np.savez(dst, **out)
    else:
        c = case(mode, name)
        cus = 0
        if device and c["packed"]:
            import torch
            cus = torch.cuda.get_device_properties(0).multi_processor_count
        num, den = accumulate(c, device)
        np.savez(dst, num=num, den=den, shape=[launch_shape(mode)[k] for k in SHAPE_KEYS] if device else [0] * 5, cus=cus)
