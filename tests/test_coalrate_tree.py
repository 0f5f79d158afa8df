"""`CoalRate --mode tree` on the CPU: the CLI with the host twin against the reference's .coal for every committed fixture
(tests/golden/crtree_*), the host twin against the numpy restatement of coal_tree::populate on random inputs with ties and
boundary-equal times, the smallest tree, weight-0 trees, the chunk cap across block boundaries, and the errors."""
import os
import shutil

import numpy as np
import pytest

import colate_amd
import coalrate_lib as cl
import coalrate_tree_lib as tl
import coalrate_tree_model as tm


def test_fixture_set():
    assert tl.CASES == tl.EXPECTED_CASES


@pytest.mark.parametrize("name", tl.EXPECTED_CASES)
def test_cli_host_twin_matches_reference(name, tmp_path):
    r = tl.run_case(name, str(tmp_path / "out"), device=False, extra_env={"COLATE_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "host twin" in r.stderr, r.stderr[-1000:]
    expected = os.path.join(tl.case_dir(name), "expected.coal")
    total, differ = cl.compare_coal(str(tmp_path / "out.coal"), expected)
    print(f"{name}: {total} rate tokens, {differ} not identical")
    if name in ("chr", "blocks"):
        # the bootstrap draws in 0 .. num_blocks: rows differ, which they cannot when every block is drawn once
        with open(expected) as f:
            rows = [ln.split(" ", 2)[2] for ln in f.read().splitlines()[2:]]
        assert len(rows) >= 4 and len(set(rows)) > 1


within_bound = tm.within_bound   # (shared with test_coalrate_edges_cpu.py)


# N, T, blocks, ancient, quantum, epochs
MODEL_SHAPES = [
    (2, 30, 3, False, None, None),
    (2, 30, 2, False, 64.0, tl.TIE_EPOCHS),
    (9, 120, 4, True, None, None),
    (33, 40, 3, True, 64.0, tl.TIE_EPOCHS),      # ties; node times equal to epoch boundaries
    (150, 12, 2, False, 64.0, tl.TIE_EPOCHS),    # more pieces in an epoch than partial sums
    (150, 12, 3, True, None, None),
]


@pytest.mark.parametrize("N,T,nb,ancient,quantum,epochs", MODEL_SHAPES)
def test_host_twin_matches_model(N, T, nb, ancient, quantum, epochs):
    rng = np.random.default_rng(31 * N + T + ancient)
    epochs = cl.bins_epochs(2.0, 6.0, 0.25) if epochs is None else epochs
    parents, bl, weights, blocks, ages = tl.random_input(rng, N, T, nb, ancient, epochs, quantum)
    if quantum:
        times = np.concatenate([tm.node_times(parents[k], bl[k], ages) for k in range(T)])
        assert np.isin(epochs[1:-1], times).sum() >= (2 if N >= 33 else 1)   # node times equal epoch boundaries
        internal = np.concatenate([tm.node_times(parents[k], bl[k], ages)[N:] for k in range(T)])
        assert N == 2 or len(np.unique(internal)) < internal.size       # ties among internal nodes
        if ancient:
            assert np.isin(ages[ages > 0], internal).any()             # and between an internal node and a sample age
    num, den = colate_amd.coalrate_tree_accumulate(parents, bl, weights, blocks, nb, epochs, ages, device=False)
    mnum, mden, n_num, n_den = tm.accumulate(parents, bl, weights, blocks, nb, epochs, ages)
    assert (mnum != 0).any() and (mden != 0).any()
    assert ((num == 0) == (mnum == 0)).all() and ((den == 0) == (mden == 0)).all()
    assert within_bound(num, mnum, n_num) and within_bound(den, mden, n_den)
    print(f"N {N}: {(num != mnum).sum()} numerators and {(den != mden).sum()} denominators differ in their last bits")


def test_smallest_tree_by_hand():
    # N = 2: leaves at 0, the root at 100 with epochs 0, 64, 128, 1e7: two lineages over [0, 64] and [64, 100]
    parents = np.array([[2, 2, -1]], dtype=np.int32)
    bl = np.array([[100.0, 100.0, 0.0]])
    num, den = colate_amd.coalrate_tree_accumulate(parents, bl, [3000.0], [0], 1, [0.0, 64.0, 128.0, 1e7], device=False)
    assert num.tolist() == [[0.0, 3000.0 / 1e9, 0.0, 0.0]]
    assert den.tolist() == [[3000.0 * 2 * 1 / 2.0 * 64.0 / 1e9, 3000.0 * 2 * 1 / 2.0 * 36.0 / 1e9, 0.0, 0.0]]


def test_all_ancient_first_piece_starts_at_zero():
    # both samples at age 10: the reference's running lower age starts at epochs[0], not at the first node
    parents = np.array([[2, 2, -1]], dtype=np.int32)
    bl = np.array([[20.0, 20.0, 0.0]])
    num, den = colate_amd.coalrate_tree_accumulate(parents, bl, [1e9], [0], 1, [0.0, 64.0, 1e7], [10.0, 10.0], device=False)
    assert den.tolist() == [[1e9 * 2 * 1 / 2.0 * 10.0 / 1e9 + 1e9 * 2 * 1 / 2.0 * 20.0 / 1e9, 0.0, 0.0]]
    assert num.tolist() == [[1.0, 0.0, 0.0]]


def test_zero_weight_tree_adds_nothing():
    rng = np.random.default_rng(5)
    epochs = cl.bins_epochs(2.0, 6.0, 0.25)
    parents, bl, weights, blocks, ages = tl.random_input(rng, 12, 20, 2, False, epochs)
    weights[[3, 4, 11]] = 0.0
    num, den = colate_amd.coalrate_tree_accumulate(parents, bl, weights, blocks, 2, epochs, device=False)
    keep = weights != 0.0
    num2, den2 = colate_amd.coalrate_tree_accumulate(parents[keep], bl[keep], weights[keep], blocks[keep], 2, epochs, device=False)
    assert np.array_equal(num.view(np.uint64), num2.view(np.uint64)) and np.array_equal(den.view(np.uint64), den2.view(np.uint64))


def test_zero_weight_trees_advance_the_block_counter(tmp_path):
    # `blocks`: 5003 trees, of which those without SNPs weigh 0: were they not counted, the first chromosome would stay
    # within one block and the reference's rows would not be reproduced; here the count is made explicit
    import gzip
    d = tl.case_dir("blocks")
    with gzip.open(os.path.join(d, "in_chr1.mut.gz"), "rt") as f:
        with_snps = len({int(r.split(";")[4]) for r in f.read().splitlines()[1:]})
    assert with_snps < 5000 < 5003
    r = tl.run_case("blocks", str(tmp_path / "out"), device=False)
    assert r.returncode == 0
    assert (tmp_path / "out.coal").read_text() == open(os.path.join(d, "expected.coal")).read()


def test_chunk_cap_crosses_blocks(tmp_path):
    rng = np.random.default_rng(9)
    epochs = cl.bins_epochs(2.0, 6.0, 0.25)
    inp = tl.random_input(rng, 10, 57, 5, True, epochs)
    a = tl.accumulate_in_child(tmp_path, inp, 5, epochs, device=False, timeout=120, chunk_trees=7)
    b = tl.accumulate_in_child(tmp_path, inp, 5, epochs, device=False, timeout=120)
    assert tl.chunk_straddles_blocks(inp[3], 7)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    r = tl.run_case("blocks", str(tmp_path / "capped"), device=False, extra_env={"COLATE_COALRATE_CHUNK_TREES": "999"})
    assert r.returncode == 0
    assert (tmp_path / "capped.coal").read_text() == open(os.path.join(tl.case_dir("blocks"), "expected.coal")).read()


def test_accumulate_errors():
    epochs = [0.0, 64.0, 128.0]
    parents = np.array([[2, 2, -1]], dtype=np.int32)
    with pytest.raises(colate_amd.ColateError, match="older than the last epoch"):
        colate_amd.coalrate_tree_accumulate(parents, [[200.0, 200.0, 0.0]], [1.0], [0], 1, epochs, device=False)
    colate_amd.coalrate_tree_accumulate(parents, [[128.0, 128.0, 0.0]], [1.0], [0], 1, epochs, device=False)  # on the boundary
    for bad in ([[2, 2, 2]], [[1, 2, -1]], [[2, -1, -1]]):
        with pytest.raises(colate_amd.ColateError):
            colate_amd.coalrate_tree_accumulate(np.array(bad, dtype=np.int32), [[1.0, 1.0, 0.0]], [1.0], [0], 1, epochs, device=False)
    with pytest.raises(colate_amd.ColateError):
        colate_amd.coalrate_tree_accumulate(parents, [[1.0, 1.0, 0.0]], [1.0], [3], 1, epochs, device=False)


def test_cli_errors(tmp_path):
    d = tl.case_dir("modern")
    for f in os.listdir(d):
        shutil.copy(os.path.join(d, f), tmp_path)
    args = ["--mode", "tree", "-i", "in", "-o", "out", "--bins", "3,6.5,0.5"]

    def fails(a, text):
        r = cl.run_cli(a, str(tmp_path), device=False)
        assert r.returncode != 0, (a, r.stdout, r.stderr)
        assert text in r.stderr + r.stdout, (text, r.stdout, r.stderr)
        assert not os.path.exists(tmp_path / "out.coal")

    fails(args + ["--coal", "x.coal"], "Option 'coal' does not exist")
    fails([a if a != "in" else "nothere" for a in args], "--mode tree: failed to open nothere_chr1.anc(.gz)")
    fails(args[:-2], "Not enough arguments supplied.")
    fails(["--mode", "trees"] + args[2:], "tree, local_ancestry.")
    os.remove(tmp_path / "in_chr1.mut.gz")
    fails(args, "--mode tree: failed to open in_chr1.mut(.gz)")
    # --poplabels and --seed are accepted and ignored
    for f in os.listdir(d):
        shutil.copy(os.path.join(d, f), tmp_path)
    r = cl.run_cli(args + ["--poplabels", "none.txt", "--seed", "4"], str(tmp_path), device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "out.coal").read_text() == open(os.path.join(d, "expected.coal")).read()
    r = cl.run_cli(["--help"], str(tmp_path), device=False)
    assert "tree, local_ancestry" in r.stdout
