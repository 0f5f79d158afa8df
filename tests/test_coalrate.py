"""`CoalRate --mode local_ancestry` on the host (no GPU needed): the CLI's host twin against the reference's .coal for every
committed fixture, the raw sums against a pair-by-pair restatement of coal_LA::populate, the 5000-tree block counter and
the bootstrap on a generated input, the two poplabels formats against each other, and the errors."""
import gzip
import os
import shutil

import numpy as np
import pytest

import coalrate_lib as cl
import coalrate_model as cm
import colate_amd


@pytest.mark.parametrize("name", cl.CASES)
def test_cli_host_matches_reference(name, tmp_path):
    r = cl.run_case(name, str(tmp_path / "out"), device=False)
    assert r.returncode == 0, r.stderr
    total, differ = cl.compare_coal(str(tmp_path / "out.coal"), os.path.join(cl.case_dir(name), "expected.coal"))
    print(f"{name}: {total} rate tokens, {differ} not identical")
    assert total > 0


def test_fixture_cases_present():
    assert set(cl.CASES) >= {"modern", "ancient", "chr", "localanc", "large", "settings"}


@pytest.mark.parametrize("ancient", [False, True])
def test_host_twin_matches_pairwise_model(ancient, monkeypatch):
    """Several group vectors and blocks, a block boundary in the middle of a chunk (chunks of 4 trees, blocks change at
    trees that are no multiples of 4)."""
    monkeypatch.setenv("COLATE_COALRATE_CHUNK_TREES", "4")
    rng = np.random.default_rng(17 + ancient)
    N, T, G, S, nb = 26, 11, 3, 3, 3
    epochs = cl.bins_epochs(2.0, 5.0, 0.25)
    parents, bl, w, blocks, gv, groups, ages = cl.random_input(rng, N, T, G, S, nb, ancient, epochs)
    blocks[:] = [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2]
    w[3] = 0.0
    num, den = colate_amd.coalrate_accumulate(parents, bl, w, blocks, nb, gv, groups, G, epochs, ages, device=False)
    model = cm.Model(epochs, nb, G)
    for t in range(T):
        model.populate(parents[t], bl[t], float(w[t]), groups[gv[t]], int(blocks[t]), ages)
    worst = cm.check_against(model, num, den)
    print(f"ancient={ancient}: largest |difference| / bound = {worst:.3g}")
    assert np.abs(num).sum() > 0 and np.abs(den).sum() > 0
    if ancient:
        assert len({int(np.searchsorted(epochs[1:], a, side="right")) for a in ages}) >= 2


class Mt19937:
    """std::mt19937 (seeded as its seed(value) does)."""

    def __init__(self, seed):
        self.x = [0] * 624
        self.x[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.x[i] = (1812433253 * (self.x[i - 1] ^ (self.x[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.p = 624

    def __call__(self):
        if self.p >= 624:
            x = self.x
            for i in range(624):
                y = (x[i] & 0x80000000) | (x[(i + 1) % 624] & 0x7FFFFFFF)
                x[i] = x[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.p = 0
        y = self.x[self.p]
        self.p += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def uniform_int(rng, n):
    """std::uniform_int_distribution<int>(0, n-1) over a 32-bit generator as libstdc++ 11 draws it (Lemire's method)."""
    prod = rng() * n
    low = prod & 0xFFFFFFFF
    if low < n:
        threshold = (2 ** 32 - n) % n
        while low < threshold:
            prod = rng() * n
            low = prod & 0xFFFFFFFF
    return prod >> 32


def fmt(x):
    if x != x:
        return "-nan"
    return "%g" % x


def write_small_genome(prefix, rng, N, T):
    """One SNP per tree, 100 bases apart; returns parents, branch lengths and every tree's weight as NextTree gives it."""
    parents, bls = [], []
    with gzip.open(prefix + ".anc.gz", "wt") as f:
        f.write(f"NUM_HAPLOTYPES {N}\nNUM_TREES {T}\n")
        for t in range(T):
            p, b = cl.random_tree(rng, N, Ne=3000.0)
            b = np.round(b, 5)
            parents.append(p)
            bls.append(b)
            f.write(f"{1000 + 100 * t}: " + " ".join(f"{int(p[v])}:({b[v]:.5f} 0.000 0 0)" for v in range(2 * N - 1)) + " \n")
    with gzip.open(prefix + ".mut.gz", "wt") as f:
        f.write("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n")
        for t in range(T):
            f.write(f"{t};{1000 + 100 * t};{100 if t + 1 < T else 1};rs{t};{t};0;0;0;10;100;A/G;A;G;\n")
    w = np.full(T, 100.0)
    w[0] = 50.0
    w[-1] = 51.0
    return np.array(parents), np.array(bls), w


def test_block_counter_and_bootstrap_beyond_5000_trees(tmp_path):
    rng = np.random.default_rng(23)
    N, T, G, boots = 6, 5203, 2, 3
    parents, bls, w = write_small_genome(str(tmp_path / "in"), rng, N, T)
    with open(tmp_path / "pop.txt", "w") as f:
        f.write("sample population group sex\n")
        for i, g in enumerate(["B", "A", "B", "A", "A", "B"]):
            f.write(f"S{i} {g} R 1\n")
    group = np.array([1, 0, 1, 0, 0, 1])
    r = cl.run_cli(["--mode", "local_ancestry", "-i", "in", "-o", "out", "--poplabels", "pop.txt", "--bins", "3,6,0.5",
                    "--num_bootstraps", str(boots)], str(tmp_path), device=False)
    assert r.returncode == 0, r.stderr
    epochs = cl.bins_epochs(3.0, 6.0, 0.5)
    nb = T // 5000 + 1
    model = cm.Model(epochs, nb, G)
    for t in range(T):
        model.populate(parents[t], bls[t], float(w[t]), group, t // 5000)
    assert model.n_num[1].sum() == 203 * 15
    mt = Mt19937(1)
    lines = ["A B ", " ".join(fmt(e) for e in epochs) + " "]
    for _ in range(boots):
        times = [0] * nb
        for _b in range(nb):
            times[uniform_int(mt, nb)] += 1
        bn = sum(times[b] * model.num[b] for b in range(nb))
        bd = sum(times[b] * model.den[b] for b in range(nb))
        for i in range(G):
            for j in range(G):
                g1, g2 = max(i, j), min(i, j)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rates = bn[g1, g2] / bd[g1, g2]
                lines.append(f"{i} {j} " + " ".join(fmt(x) for x in rates) + " ")
    with open(tmp_path / "model.coal", "w") as f:
        f.write("\n".join(lines) + "\n")
    total, differ = cl.compare_coal(str(tmp_path / "out.coal"), str(tmp_path / "model.coal"))
    print(f"{total} rate tokens, {differ} not identical")


def test_two_poplabels_formats_agree(tmp_path):
    src = cl.case_dir("chr")
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    args = ["--mode", "local_ancestry", "-i", "in", "--chr", "chr.txt", "--bins", "3,6.5,0.5", "--num_bootstraps", "2"]
    r = cl.run_cli(args + ["-o", "four", "--poplabels", "pop.txt"], str(tmp_path), device=False)
    assert r.returncode == 0, r.stderr
    assert "Assuming 4 column poplabels file" in r.stderr
    with open(tmp_path / "pop.txt") as f:
        rows = [ln.split() for ln in f.read().splitlines()[1:]]
    names = sorted({row[1] for row in rows})
    hap = []
    for row in rows:
        hap += [names.index(row[1])] * (1 if row[3] == "1" else 2)
    with open(tmp_path / "la.txt", "w") as f:
        f.write(" ".join(names) + "\n")
        for c in ("1", "2", "X"):
            f.write(f"{c} 0 " + " ".join(map(str, hap)) + "\n")
    r = cl.run_cli(args + ["-o", "la", "--poplabels", "la.txt"], str(tmp_path), device=False)
    assert r.returncode == 0, r.stderr
    assert "Assuming loc ancestry poplabels file" in r.stderr
    with open(tmp_path / "four.coal") as a, open(tmp_path / "la.coal") as b:
        assert a.read() == b.read()


def _modern_args(tmp_path):
    src = cl.case_dir("modern")
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    return ["--mode", "local_ancestry", "-i", "in", "-o", "out", "--poplabels", "pop.txt", "--bins", "3,6.5,0.5"]


def test_errors(tmp_path):
    args = _modern_args(tmp_path)
    cwd = str(tmp_path)

    def fails(a, text):
        r = cl.run_cli(a, cwd, device=False)
        assert r.returncode != 0, (a, r.stdout, r.stderr)
        assert text in r.stderr + r.stdout, (text, r.stdout, r.stderr)
        assert not os.path.exists(tmp_path / "out.coal")

    fails(args + ["--coal", "x.coal"], "Option 'coal' does not exist")
    fails(["--mode", "tree"] + args[2:], "--mode tree")
    fails(args[:-2], "Not enough arguments supplied.")
    # the local ancestry format: a chromosome's first row not at bp 0, a label row of the wrong length
    labels = "PA PB PC PD"
    with open(tmp_path / "la.txt", "w") as f:
        f.write(labels + "\nNA 5 " + " ".join(["0"] * 40) + "\n")
    la = [a if a != "pop.txt" else "la.txt" for a in args]
    fails(la, "First entry for new chr has to start at BP = 0")
    with open(tmp_path / "la.txt", "w") as f:
        f.write(labels + "\nNA 0 " + " ".join(["0"] * 40) + "\nNA 90000 " + " ".join(["1"] * 39) + "\n")
    fails(la, "39 labels")
    with open(tmp_path / "la.txt", "w") as f:
        f.write(labels + "\nNA 0 " + " ".join(["0"] * 38) + "\n")
    fails(la, "38 labels")
    # a node beyond the last epoch boundary (10^8 / years_per_gen^2 generations with these bins)
    b = [a if a != "3,6.5,0.5" else "1,2,0.5" for a in args] + ["--years_per_gen", "40000"]
    fails(b, "older than the last epoch boundary")


def test_abi_rejects_node_beyond_last_epoch():
    rng = np.random.default_rng(3)
    parents, bl = cl.random_tree(rng, 8)
    with pytest.raises(colate_amd.ColateError, match="older than the last epoch boundary"):
        colate_amd.coalrate_accumulate(parents[None], bl[None], [1.0], [0], 1, [0], np.zeros((1, 8), dtype=np.int32), 1,
                                       [0.0, 1e-3, 2e-3], device=False)


def test_abi_rejects_node_in_an_epoch_below_a_sample_age_under_it():
    """A zero-length branch above a sample whose age lies exactly on an epoch boundary: the node's time equals the boundary,
    so the node belongs to the epoch below it and the sample's age to the epoch above."""
    epochs = [0.0, 10.0, 100.0, 1e6]
    parents = np.array([[3, 3, 4, 4, -1]], dtype=np.int32)
    bl = np.array([[0.0, 10.0, 50.0, 40.0, 0.0]])
    ages = [10.0, 0.0, 0.0]
    groups = np.zeros((1, 3), dtype=np.int32)
    with pytest.raises(colate_amd.ColateError, match="epoch below that of a sample age under it"):
        colate_amd.coalrate_accumulate(parents, bl, [1.0], [0], 1, [0], groups, 1, epochs, ages, device=False)
    # the same tree with the sample just below the boundary is accepted
    num, den = colate_amd.coalrate_accumulate(parents, bl, [1.0], [0], 1, [0], groups, 1, epochs, [9.5, 0.0, 0.0], device=False)
    assert num.sum() > 0 and den.sum() > 0


def test_abi_rejects_too_many_groups():
    """G above 65535, or E * G * (G + 1) / 2 of 2^31 or more, is refused before anything is read or allocated."""
    from colate_amd._lib import lib
    one = np.zeros(8)
    for G, E in ((70000, 3), (60000, 3)):
        rc = lib.colate_coalrate_accumulate_host(3, 0, None, None, None, None, 1, None, 1, one.ctypes.data, G, None, E,
                                                 one.ctypes.data, one.ctypes.data, one.ctypes.data)
        assert rc < 0 and b"groups" in lib.colate_last_error(), (rc, lib.colate_last_error())
