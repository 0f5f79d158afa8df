"""A literal Python restatement of GetConditionalCoalescentRate (include/coal/coal.cpp:4786-4999), TEST INFRASTRUCTURE:
per focal haplotype, per conditional haplotype, per member of every sibling subtree, as the reference loops -- float32
coordinates, ages, epochs and addends, operand for operand -- but with the sums in float64.  It is the independent check
of the factorised walk (condcoal_walk.hpp); small inputs only."""
import numpy as np

f32 = np.float32


def _leaves(parent, N):
    nn = len(parent)
    members = [[v] if v < N else [] for v in range(nn)]
    children = [[] for _ in range(nn)]
    for v in range(nn):
        if parent[v] >= 0:
            children[parent[v]].append(v)
    # children before parents, whatever the labelling: repeated passes in a topological order
    order, seen = [], [False] * nn
    stack = [nn - 1]
    while stack:
        x = stack.pop()
        if x >= 0:
            stack.append(~x)
            stack.extend(children[x])
        else:
            order.append(~x)
    for v in order:
        for c in children[v]:
            members[v] += members[c]
    return members, children


def tree_accumulators(parent, bl, factor, group_of_hap, G, focal, cond, epochs, efocal, ages=None):
    """num, denom [EF][E][G] (float64) of one tree.  cond: conditional haplotypes ([] = the empty group, [-1])."""
    N = (len(parent) + 1) // 2
    nn = 2 * N - 1
    E, EF = len(epochs), len(efocal)
    epochs = [f32(e) for e in epochs] + [f32(np.inf)]  # (one past the end reads as +inf)
    efocal = [f32(e) for e in efocal]
    factor = f32(factor)
    num = np.zeros((EF, E, G))
    den = np.zeros((EF, E, G))
    members, children = _leaves(parent, N)
    conds = list(cond) if len(cond) else [-1]
    ancient = ages is not None
    for f in focal:
        for c in conds:
            if f == c:
                continue
            node = f
            p = parent[f]
            age = float(ages[f]) if ancient else 0.0
            coal_age = f32(age)
            coord = f32(age)
            ep_coal = 0
            use = c == -1
            while True:
                if not use:
                    if c in members[node]:
                        coal_age = coord
                        use = True
                    s = 0
                    if ancient:
                        if efocal[s] < coord:
                            while efocal[s] < coord:
                                s += 1
                                if s == EF:
                                    break
                            s -= 1
                    else:
                        if efocal[s] <= coal_age:
                            while efocal[s] <= coal_age:
                                s += 1
                                if s == EF:
                                    break
                            if s > 0:
                                s -= 1
                    ep_coal = s
                coord = f32(float(coord) + float(bl[node]))
                if use:
                    sib = [x for x in children[p] if x != node][0]
                    ep_init = 0
                    if coal_age > epochs[0]:
                        while ep_init < E and coal_age > epochs[ep_init]:
                            ep_init += 1
                        ep_init -= 1
                    for x in members[sib]:
                        g = group_of_hap[x]
                        if ancient:
                            lower = f32(max(age, float(ages[x])))
                            lower = max(lower, coal_age)
                            s, ep = ep_coal, ep_init
                            if not lower <= coal_age:
                                if efocal[s] < lower:
                                    while efocal[s] < lower:
                                        s += 1
                                        if s == EF:
                                            break
                                    s -= 1
                                if epochs[ep] < lower:
                                    while epochs[ep] < lower:
                                        ep += 1
                                        if ep == E:
                                            break
                                    ep -= 1
                        else:
                            lower, s, ep = coal_age, ep_coal, ep_init
                        while coord > epochs[ep + 1]:
                            den[s, ep, g] += float(factor * f32(epochs[ep + 1] - lower))
                            ep += 1
                            lower = epochs[ep]
                        den[s, ep, g] += float(factor * f32(coord - lower))
                        num[s, ep, g] += float(factor)
                node = p
                if node == nn - 1:
                    break
                p = parent[node]
    return num, den
