"""Synthetic `Colate --mode CondCoalRates` inputs (TEST INFRASTRUCTURE), in the formats the reference reads:
Relate .anc (include/src/anc.cpp:6-45, header mutations.cpp:536-590), .mut (mutations.cpp:56-283), poplabels
(sample.cpp:8-110) and a fasta mask (data.cpp:213-235).

Trees are binary coalescent genealogies with Relate's labelling (leaves 0..N-1, internal nodes in coalescence order, root
2N-2), optionally with sample ages (ancient samples enter the genealogy at their age).  Some trees carry no SNP (weight 0),
one tree is a caterpillar, one has its internal labels shuffled (the root kept at 2N-2), and SNP positions can span more
than one 30 Mb block."""
import gzip
import os

import numpy as np


def coalescent_tree(rng, N, ages=None, Ne=5000.0):
    """parent[2N-1] (-1 at the root) and node heights, internal nodes labelled N.. in coalescence order."""
    ages = np.zeros(N) if ages is None else np.asarray(ages, float)
    order = np.argsort(ages, kind="stable")
    heights = np.zeros(2 * N - 1)
    heights[:N] = ages
    parent = np.full(2 * N - 1, -1, dtype=np.int64)
    active = []
    nxt = 0  # next sample (in age order) to enter
    t = 0.0
    label = N
    while label < 2 * N - 1:
        while nxt < N and ages[order[nxt]] <= t:
            active.append(int(order[nxt]))
            nxt += 1
        k = len(active)
        if k < 2:
            t = ages[order[nxt]]
            continue
        wait = rng.exponential(2.0 * Ne / (k * (k - 1) / 2.0))
        if nxt < N and t + wait > ages[order[nxt]]:
            t = ages[order[nxt]]
            continue
        t = round(t + wait, 2)  # (two decimals: the fixtures compress)
        i, j = rng.choice(k, size=2, replace=False)
        a, b = active[i], active[j]
        for x in sorted((i, j), reverse=True):
            active.pop(x)
        parent[a] = parent[b] = label
        heights[label] = t
        active.append(label)
        label += 1
    return parent, heights


def caterpillar_tree(rng, N, ages=None, step=40.0):
    """Leaves joined one at a time: path length N-1 from the first pair to the root."""
    ages = np.zeros(N) if ages is None else np.asarray(ages, float)
    perm = rng.permutation(N)
    parent = np.full(2 * N - 1, -1, dtype=np.int64)
    heights = np.zeros(2 * N - 1)
    heights[:N] = ages
    prev = int(perm[0])
    h = float(ages.max())
    for i in range(1, N):
        h = round(h + step * (0.5 + rng.random()), 2)
        node = N + i - 1
        parent[prev] = parent[int(perm[i])] = node
        heights[node] = h
        prev = node
    return parent, heights


def shuffle_internal(rng, parent, heights, N):
    """Relabel the internal nodes other than the root at random (parents no longer above their children in label order)."""
    nn = 2 * N - 1
    perm = np.arange(nn)
    inner = np.arange(N, nn - 1)
    perm[N:nn - 1] = rng.permutation(inner)
    newp = np.full(nn, -1, dtype=np.int64)
    newh = np.zeros(nn)
    for v in range(nn):
        newh[perm[v]] = heights[v]
        if parent[v] >= 0:
            newp[perm[v]] = perm[parent[v]]
    return newp, newh


def tree_line(pos, parent, heights):
    bl = [heights[parent[v]] - heights[v] if parent[v] >= 0 else 0.0 for v in range(len(parent))]
    return f"{pos}: " + " ".join(f"{int(parent[v])}:({bl[v]:.5f} 0.000 0 0)" for v in range(len(parent))) + " \n"


def write_chromosome(path_prefix, rng, N, num_trees, ages=None, span=40_000_000, caterpillar=None, shuffled=None,
                     no_snp_frac=0.15, gz=True, Ne=5000.0, tree_fn=None):
    """PREFIX.anc(.gz) and PREFIX.mut(.gz).  Returns the list of (tree index, #SNPs).  tree_fn(N, ages): another tree
    generator (parent, heights) for the other trees."""
    lines = []
    snps = []  # (pos, tree)
    counts = []
    # SNP counts per tree: the last tree always has SNPs
    for t in range(num_trees):
        c = 0 if (t < num_trees - 1 and rng.random() < no_snp_frac) else int(rng.integers(1, 5))
        counts.append(c)
    total = sum(counts)
    pos = np.sort(rng.choice(np.arange(1000, span), size=total, replace=False))
    k = 0
    for t in range(num_trees):
        if t == caterpillar:
            parent, heights = caterpillar_tree(rng, N, ages)
        elif tree_fn is not None:
            parent, heights = tree_fn(N, ages)
        else:
            parent, heights = coalescent_tree(rng, N, ages, Ne)
        if t == shuffled:
            parent, heights = shuffle_internal(rng, parent, heights, N)
        first = int(pos[k]) if counts[t] else (int(pos[k]) if k < total else int(pos[-1]))
        lines.append(tree_line(first, parent, heights))
        for _ in range(counts[t]):
            snps.append((int(pos[k]), t))
            k += 1
    header = f"NUM_HAPLOTYPES {N}" + ("" if ages is None else " " + " ".join(f"{a:g}" for a in ages)) + "\n"
    header += f"NUM_TREES {num_trees}\n"
    opener = (lambda p: gzip.open(p + ".gz", "wt")) if gz else (lambda p: open(p, "w"))
    with opener(path_prefix + ".anc") as f:
        f.write(header)
        f.writelines(lines)
    with opener(path_prefix + ".mut") as f:
        f.write("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n")
        for i, (p, t) in enumerate(snps):
            dist = (snps[i + 1][0] - p) if i + 1 < len(snps) else 1
            f.write(f"{i};{p};{dist};rs{i};{t};0;0;0;10;100;A/G;A;G;\n")
    return counts


def write_poplabels(path, N, num_groups, rng, diploid=True):
    """Samples in groups G1..Gk (names sorted differently from their first appearance); N haplotypes in all."""
    names = [f"P{chr(ord('A') + i)}" for i in range(num_groups)][::-1]
    n_samples = N // 2 if diploid else N
    grp = [names[i % num_groups] if i < num_groups else names[int(rng.integers(num_groups))] for i in range(n_samples)]
    with open(path, "w") as f:
        f.write("sample population group sex\n")
        for i, g in enumerate(grp):
            f.write(f"S{i} {g} R {'NA' if diploid else 1}\n")
    hap = []
    for g in grp:
        hap += [g, g] if diploid else [g]
    return sorted(set(names)), hap


def write_mask(path, length, rng, holes=40, hole_len=60_000):
    seq = np.full(length, ord("P"), dtype=np.uint8)
    for _ in range(holes):
        a = int(rng.integers(0, max(1, length - hole_len)))
        seq[a:a + int(rng.integers(hole_len // 4, hole_len))] = ord("N")
    with gzip.open(path + ".gz", "wt") as f:
        f.write(">chr\n")
        s = seq.tobytes().decode()
        for i in range(0, length, 100):
            f.write(s[i:i + 100] + "\n")


def ancient_ages(rng, N, frac=0.3, max_age=3000.0):
    ages = np.zeros(N)
    idx = rng.choice(N, size=max(1, int(frac * N)), replace=False)
    ages[idx] = np.round(rng.uniform(50, max_age, size=idx.size), 1)
    # diploid samples: both haplotypes the same age
    ages[1::2] = ages[0::2]
    return ages
