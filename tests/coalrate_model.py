"""A literal restatement of coal_LA::populate (include/coal/coal_tree.cpp:447-527), pair by pair in the reference's order
(TEST INFRASTRUCTURE, as condcoal_model.py is), with the bookkeeping the tests' bound needs: per cell the number of
additions made into it and the sum of their absolute values."""
import numpy as np


def coordinates(parent, bl, N, ages=None):
    """Tree::GetCoordinates (anc.cpp:280-321): float32 node times, a parent at max(child + branch length)."""
    nn = 2 * N - 1
    kids = [[] for _ in range(nn)]
    for v in range(nn):
        if parent[v] >= 0:
            kids[parent[v]].append(v)
    t = np.zeros(nn, dtype=np.float32)
    if ages is not None:
        t[:N] = np.asarray(ages, dtype=np.float32)
    done = np.zeros(nn, dtype=bool)
    done[:N] = True
    stack = [nn - 1]
    while stack:
        v = stack[-1]
        pend = [c for c in kids[v] if not done[c]]
        if pend:
            stack.extend(pend)
            continue
        stack.pop()
        if v >= N:
            t[v] = np.float32(max(float(t[c]) + float(bl[c]) for c in kids[v]))
        done[v] = True
    return t, kids


def leaves_below(kids, N):
    nn = 2 * N - 1
    out = [None] * nn

    def rec(v):
        if v < N:
            out[v] = [v]
        else:
            out[v] = []
            for c in kids[v]:
                rec(c)
                out[v] += out[c]
    import sys
    sys.setrecursionlimit(100000)
    rec(nn - 1)
    return out


class Model:
    def __init__(self, epochs, num_blocks, G):
        self.epochs = [float(e) for e in epochs]
        E = len(self.epochs)
        shape = (num_blocks, G, G, E)
        self.num = np.zeros(shape)
        self.den = np.zeros(shape)
        self.n_num = np.zeros(shape, dtype=np.int64)
        self.n_den = np.zeros(shape, dtype=np.int64)
        self.abs_num = np.zeros(shape)
        self.abs_den = np.zeros(shape)

    def _add(self, which, idx, v):
        arr, n, ab = (self.num, self.n_num, self.abs_num) if which == "num" else (self.den, self.n_den, self.abs_den)
        arr[idx] += v
        n[idx] += 1
        ab[idx] += abs(v)

    def populate(self, parent, bl, w, group, block, ages=None):
        epochs = self.epochs
        E = len(epochs)
        N = (len(parent) + 1) // 2
        coords, kids = coordinates(parent, bl, N, ages)
        desc = leaves_below(kids, N)
        order = sorted(range(2 * N - 1), key=lambda i: (float(coords[i]), i))
        ep = 1
        tmpl = [0.0] * E
        lower = 0.0
        for v in order:
            c = float(coords[v])
            while c > epochs[ep]:
                tmpl[ep - 1] += (epochs[ep] - lower) * w / 1e9
                lower = epochs[ep]
                ep += 1
            tmpl[ep - 1] += (c - lower) * w / 1e9
            lower = c
            if len(desc[v]) > 1:
                c1, c2 = kids[v]
                for m1 in desc[c1]:
                    for m2 in desc[c2]:
                        age = 0.0 if ages is None else max(float(ages[m1]), float(ages[m2]))
                        g1, g2 = int(group[m1]), int(group[m2])
                        if g2 > g1:
                            g1, g2 = g2, g1
                        self._add("num", (block, g1, g2, ep - 1), w / 1e9)
                        ep_tmp = 1
                        exceeded = False
                        for e in range(E):
                            if ep_tmp < E and epochs[ep_tmp] > age:
                                self._add("den", (block, g1, g2, e), tmpl[e])
                                if not exceeded:
                                    self._add("den", (block, g1, g2, e), -((age - epochs[ep_tmp - 1]) * w / 1e9))
                                    exceeded = True
                            ep_tmp += 1
                            if tmpl[e] == 0.0:
                                break


def check_against(model, num, den):
    """Per cell |value - model| <= 4 n 2^-53 * (the sum of the model's absolute addends), n the model's additions there: the
    worst-case rounding of the reference's own summation.  Returns the largest ratio to the bound seen."""
    worst = 0.0
    for got, ref, n, ab in ((num, model.num, model.n_num, model.abs_num), (den, model.den, model.n_den, model.abs_den)):
        bound = 4.0 * n * 2.0 ** -53 * ab
        diff = np.abs(got - ref)
        bad = diff > bound
        assert not bad.any(), (np.argwhere(bad)[:5], diff[bad][:5], bound[bad][:5])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, diff / bound, 0.0)
        worst = max(worst, float(r.max()))
    return worst
