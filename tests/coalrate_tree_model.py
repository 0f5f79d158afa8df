"""A numpy restatement of coal_tree::populate (TEST INFRASTRUCTURE; include/coal/coal_tree.cpp:100-178): the node times in
float32, the sort by (time, label), num_lins per tie group, and the walk against the epoch boundaries that adds piece by
piece, in the reference's order, straight into the block's sums."""
import numpy as np


def node_times(parent, bl, ages=None):
    """Tree::GetCoordinates: float32 times, a node at the float of max(child time + branch length)."""
    nn = len(parent)
    N = (nn + 1) // 2
    t = np.zeros(nn, dtype=np.float32)
    if ages is not None:
        t[:N] = np.asarray(ages, dtype=np.float32)
    best = np.full(nn, -np.inf)
    pending = np.full(nn, 2)
    queue = list(range(N))
    for x in queue:
        p = int(parent[x])
        if p < 0:
            continue
        best[p] = max(best[p], float(t[x]) + float(bl[x]))
        pending[p] -= 1
        if pending[p] == 0:
            t[p] = np.float32(best[p])
            queue.append(p)
    return t


def populate(t, w, epochs, num, den, n_num, n_den):
    """Adds one tree (times t, weight w) to num / den [E]; n_num / n_den count the addends of every cell."""
    nn = len(t)
    N = (nn + 1) // 2
    w = float(w)
    order = np.lexsort((np.arange(nn), t))
    st = t[order]
    scan = np.cumsum(np.where(order < N, 1, -1))
    lins = scan[np.searchsorted(st, st, side="right") - 1]     # the count once every node of the tie group is in
    k, cell, lower = 1, 0, float(epochs[0])
    for ei in range(1, len(epochs)):
        bound = float(epochs[ei])
        while float(st[k]) <= bound:
            if order[k] >= N:
                num[cell] += w / 1e9
                n_num[cell] += 1
            L = int(lins[k - 1])
            den[cell] += w * L * (L - 1) / 2.0 * (float(st[k]) - lower) / 1e9
            n_den[cell] += 1
            lower = float(st[k])
            k += 1
            if k == nn:
                return
        L = int(lins[k - 1])
        den[cell] += w * L * (L - 1) / 2.0 * (bound - lower) / 1e9
        n_den[cell] += 1
        lower = bound
        cell += 1
    raise ValueError("a node is older than the last epoch boundary")


def accumulate(parents, bl, weights, blocks, num_blocks, epochs, ages=None):
    E = len(epochs)
    num = np.zeros((num_blocks, E))
    den = np.zeros((num_blocks, E))
    n_num = np.zeros((num_blocks, E), dtype=np.int64)
    n_den = np.zeros((num_blocks, E), dtype=np.int64)
    for k in range(len(weights)):
        b = int(blocks[k])
        populate(node_times(parents[k], bl[k], ages), weights[k], epochs, num[b], den[b], n_num[b], n_den[b])
    return num, den, n_num, n_den


def within_bound(a, b, n):
    """|a - b| <= 2 n 2^-53 max(a, b): all addends are non-negative and formed by the same expression, so every summation
    order is within (n - 1) 2^-53 of the exact sum (relative)."""
    return (np.abs(a - b) <= 2.0 * n * 2.0 ** -53 * np.maximum(a, b)).all()
