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


def _hit(events, key, n=1):
    if events is not None:
        events[key] = events.get(key, 0) + n


def tree_accumulators(parent, bl, factor, group_of_hap, G, focal, cond, epochs, efocal, ages=None, events=None):
    """num, denom [EF][E][G] (float64) of one tree.  cond: conditional haplotypes ([] = the empty group, [-1]).
    events: an optional dict that counts, per key, how often the walk met an edge (a coordinate on a boundary, a search
    that ran off its vector, ...): what an input exercises, counted where it happens.  The sums do not depend on it."""
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
        joins = {}  # ancestor at which a conditional joins f's lineage -> how many do (the walk's class weight m)
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
                        joins[node] = joins.get(node, 0) + 1
                        if coal_age in efocal[1:]:
                            _hit(events, "ancient_coal_age_on_focal_boundary" if ancient else "modern_coal_age_on_focal_boundary")
                    s = 0
                    if ancient:
                        if efocal[s] < coord:
                            while efocal[s] < coord:
                                s += 1
                                if s == EF:
                                    if use:
                                        _hit(events, "focal_search_hits_EF")
                                    break
                            s -= 1
                    else:
                        if efocal[s] <= coal_age:
                            while efocal[s] <= coal_age:
                                s += 1
                                if s == EF:
                                    if use:
                                        _hit(events, "focal_search_hits_EF")
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
                        if ep_init == E:
                            _hit(events, "epoch_search_hits_E")
                        ep_init -= 1
                    if events is not None:
                        if coord in epochs[1:E]:
                            _hit(events, "coord_on_epoch_boundary")
                        if coal_age in epochs[1:E]:
                            _hit(events, "coal_age_on_epoch_boundary")
                        if float(bl[node]) == 0.0:
                            _hit(events, "zero_branch_on_used_step")
                        if not ancient:
                            _hit(events, "modern_sibling_smaller_than_G" if len(members[sib]) < G else "modern_sibling_at_least_G")
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
                                            _hit(events, "focal_search_hits_EF")
                                            break
                                    s -= 1
                                if epochs[ep] < lower:
                                    while epochs[ep] < lower:
                                        ep += 1
                                        if ep == E:
                                            _hit(events, "epoch_search_hits_E")
                                            break
                                    ep -= 1
                                if events is not None:
                                    tag = "empty_cond" if c == -1 else "nonempty_cond"
                                    _hit(events, f"ancient_lower_above_coal_age_{tag}")
                                    if s != ep_coal:
                                        _hit(events, f"ancient_lower_advances_s_{tag}")
                                    if ep != ep_init:
                                        _hit(events, f"ancient_lower_advances_ep_{tag}")
                                    if lower in efocal[1:]:
                                        _hit(events, "ancient_lower_on_focal_boundary")
                                    if lower in epochs[1:E]:
                                        _hit(events, "ancient_lower_on_epoch_boundary")
                        else:
                            lower, s, ep = coal_age, ep_coal, ep_init
                        while coord > epochs[ep + 1]:
                            den[s, ep, g] += float(factor * f32(epochs[ep + 1] - lower))
                            ep += 1
                            lower = epochs[ep]
                        if ep + 1 == E:
                            _hit(events, "epoch_past_the_end_read_as_inf")
                        den[s, ep, g] += float(factor * f32(coord - lower))
                        num[s, ep, g] += float(factor)
                node = p
                if node == nn - 1:
                    break
                p = parent[node]
        _hit(events, "class_weight_above_one", sum(1 for m in joins.values() if m > 1))
    return num, den
