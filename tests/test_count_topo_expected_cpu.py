"""colate_topo_expected_blocks without a device, and `Colate --mode count_topo --samples --age_profile --expected` on the host twin
and on the cursor path: the twin against the contract restated in Python integers (count_topo_expected_lib.model), against the
reference's own lines where target and reference are fixed, against the sampled counts on pseudo-haploid inputs, regrouped across
block sizes, the quotient against Python's `//`, the refusals by message, and the files of the command line."""
import numpy as np
import pytest

import colate_amd
import count_topo_expected_lib as xl
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl

EPOCHS = jl.epochs_sets()
WHOLE = 1000 * jl.B  # one block per chromosome of the edge case


def qualifying_of_the_profile(c, epochs, nbpb):
    _, counts, _ = jl.profile_blocks(c, epochs, nbpb, device=False)
    return counts[..., 2].copy()


# ------------------------------------------------------------------ 1. the twin against the model
@pytest.mark.parametrize("E", sorted(EPOCHS))
@pytest.mark.parametrize("nbpb", jl.NBPB)
def test_fixture_twin_equals_the_model_in_every_integer(nbpb, E):
    case = jl.fixture_case()[0]
    blk_off, counts = xl.expected(case, EPOCHS[E], nbpb, device=False)
    assert (blk_off == jl.blocks_model(case["row_off"], case["rows"]["pos"], nbpb)).all()
    assert counts.shape == (14, int(blk_off[-1]), E, 3) and counts.dtype == np.int64
    cells = xl.model(case, EPOCHS[E], nbpb)
    xl.assert_equals_model(counts, cells)
    assert (counts[..., 2] == qualifying_of_the_profile(case, EPOCHS[E], nbpb)).all()
    assert (counts[..., 0] + counts[..., 1] <= counts[..., 2] * xl.ONE).all()
    # fractional rows are there: a third to a half of most triples' qualifying rows (3 % in `c a b`)
    assert sum(1 for v in cells.values() if v[0] % xl.ONE or v[1] % xl.ONE) > 100


@pytest.mark.parametrize("E", (1, 11, 1024))
@pytest.mark.parametrize("nbpb", (jl.B, 1, WHOLE))
def test_edge_rows_twin_equals_the_model_in_every_integer(nbpb, E):
    c = jl.edge_case()
    blk_off, counts = xl.expected(c, pl.EPOCHS[E], nbpb, device=False)
    assert counts.shape == (3, int(blk_off[-1]), E, 3)
    xl.assert_equals_model(counts, xl.model(c, pl.EPOCHS[E], nbpb))
    assert not counts[1].any() and int(counts[0, ..., 2].sum()) == jl.N0 + 1 and int(counts[2, ..., 2].sum()) == len(jl.SPARSE_ROWS)
    q = counts[..., 2].copy()
    del counts
    assert (q == qualifying_of_the_profile(c, pl.EPOCHS[E], nbpb)).all()


# ------------------------------------------------------------------ 2. the reference's own lines where T and R are fixed
def test_fixed_rows_equal_the_references_lines_for_every_fixture_triple():
    case, meta, _, _ = jl.fixture_case()
    nbpb, epochs = 5_000_000, EPOCHS[23]
    blk_off = colate_amd.topo_blocks(case["row_off"], case["rows"], nbpb)
    blk = jl.row_blocks(case, nbpb, blk_off)
    epoch = pl.age_epoch(case["rows"]["age_begin"], case["rows"]["age_end"], epochs)
    lines = jl.reference_lines()
    mixed = (case["idx"]["DAF"] > 0) & (case["idx"]["AAF"] > 0)
    assert len(meta["triples"]) == 14
    for p, t in enumerate(case["triples"]):
        T, R = int(t["target"]), int(t["reference"])
        drop = mixed[T] | mixed[R]
        idx = case["idx"].copy()
        for s in (T, R):
            idx["DAF"][s][drop], idx["AAF"][s][drop] = 0, 0
        alone = dict(case, idx=idx, triples=case["triples"][p:p + 1])
        _, counts = xl.expected(alone, epochs, nbpb, device=False)
        assert 178 <= int(counts[..., 2].sum()) <= 779, (p, int(counts[..., 2].sum()))
        assert not (counts[..., :2] % xl.ONE).any()
        want = np.zeros(counts.shape[1:3] + (2,), dtype=np.int64)
        for q, g, sign in lines:
            if q == p and not drop[g]:
                want[blk[g], epoch[g], 0 if sign > 0 else 1] += 1
        assert want[..., 0].sum() >= 30 and want[..., 1].sum() >= 30, (p, want.sum(axis=(0, 1)))  # (it cannot pass empty)
        assert (counts[0, :, :, :2] // xl.ONE == want).all(), (p, meta["triples"][p]["names"])
        if meta["triples"][p]["names"] == ["a", "b", "c"]:
            assert want.sum(axis=(0, 1)).tolist() == [59, 39]


# ------------------------------------------------------------------ 3. pseudo-haploid inputs: the sampled counts themselves
def test_pseudo_haploid_inputs_give_the_sampled_counts_whatever_the_uniforms():
    c = jl.edge_case()
    idx = c["idx"].copy()
    idx["AAF"][idx["DAF"] > 0] = 0
    rng = np.random.default_rng(3)
    ep = pl.EPOCHS[11]
    _, counts = xl.expected(dict(c, idx=idx), ep, jl.B, device=False)
    assert counts[..., 0].sum() > 100 * xl.ONE and counts[..., 1].sum() > 100 * xl.ONE
    for u in (c["uniforms"], rng.uniform(size=c["uniforms"].size)):
        _, sampled, _ = jl.profile_blocks(dict(c, idx=idx, uniforms=u), ep, jl.B, device=False)
        assert (counts[..., :2] == xl.ONE * sampled[..., :2]).all() and (counts[..., 2] == sampled[..., 2]).all()


# ------------------------------------------------------------------ 4. regrouping
def test_finer_blocks_regrouped_are_the_coarser_ones():
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    fine, mid, whole = (xl.expected(c, ep, nbpb, device=False) for nbpb in (1, jl.B, WHOLE))
    assert 10_000 < fine[0][-1] <= 65535 and np.diff(whole[0]).tolist() == [1, 1, 1]
    assert (jl.regroup(fine[1], fine[0], 1, mid[0], jl.B) == mid[1]).all()
    assert (jl.regroup(mid[1], mid[0], jl.B, whole[0], WHOLE) == whole[1]).all()
    assert (jl.regroup(fine[1], fine[0], 1, whole[0], WHOLE) == whole[1]).all()
    assert whole[1][0, ..., :2].sum() > 0


# ------------------------------------------------------------------ 5. the quotient
def per_row(c):
    """[rows][3] of a one-triple case whose rows lie at distinct positions 1 + 3 k: one base per block, one epoch"""
    _, counts = xl.expected(c, [0.0], 1, device=False)
    return counts[0, (c["rows"]["pos"] - 1).astype(np.int64), 0, :]


def test_addends_equal_pythons_floor_division():
    small = [(a, b, d, e) for a in range(9) for b in range(9) for d in range(9) for e in range(9) if a + b > 0 and d + e > 0]
    n = len(small)
    assert n == 80 * 80
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"] = 1 + 3 * np.arange(n)
    idx = np.zeros((3, n), dtype=colate_amd.WALK_IDX)
    idx["DAF"][0] = 1
    at = np.array(small)
    idx["DAF"][1], idx["AAF"][1], idx["DAF"][2], idx["AAF"][2] = at[:, 0], at[:, 1], at[:, 2], at[:, 3]
    c = dict(row_off=np.array([0, n], dtype=np.int64), rows=rows, idx=idx, cond_idx=idx.copy(), triples=np.array([(0, 1, 2)], dtype=colate_amd.TOPO_TRIPLE))
    extreme, combos = xl.extreme_case()
    for case, counts_of in ((c, small), (extreme, [(1, 1, 1, 1)] * 40 + combos + [(1, 1, 1, 1)] * 5)):
        got = per_row(case).tolist()
        assert len(got) == len(counts_of)
        for (a, b, d, e), x in zip(counts_of, got):
            want = [a * e * xl.ONE // ((a + b) * (d + e)), b * d * xl.ONE // ((a + b) * (d + e)), 1]
            assert x == want, ((a, b, d, e), x, want)
            assert x[0] + x[1] <= xl.ONE
    assert len(combos) == 256 and (65535, 65535, 65535, 65535) in combos


# ------------------------------------------------------------------ 6. the refusals
def test_refusals_by_message_and_nothing_written():
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    with pytest.raises(colate_amd.ColateError, match=r"epochs\[2\] = 1 does not lie above epochs\[1\] = 5"):
        xl.expected(c, np.array([0.0, 5.0, 1.0]), jl.B, device=False)
    with pytest.raises(colate_amd.ColateError, match="num_bases_per_block = 0: at least 1"):
        xl.expected(c, ep, 0, device=False)
    tr = c["triples"].copy()
    tr[1]["target"] = 4
    with pytest.raises(colate_amd.ColateError, match="triple 1: sample id out of range"):
        xl.expected(dict(c, triples=tr), ep, jl.B, device=False)
    lib = colate_amd.api.lib
    a = [np.ascontiguousarray(c[k]) for k in ("row_off", "rows", "idx", "cond_idx", "triples")] + [ep.copy()]
    p = [x.ctypes.data for x in a]
    nb = int(colate_amd.topo_blocks(c["row_off"], c["rows"], jl.B)[-1])
    counts = np.full((3, nb + 1, 11, 3), -7, dtype=np.int64)

    def call(nb_given, counts_p=counts.ctypes.data, epochs_p=p[5]):
        return lib.colate_topo_expected_blocks_host(3, p[0], p[1], 4, p[2], p[3], 3, p[4], 11, epochs_p, jl.B, nb_given, counts_p)

    assert call(nb + 1) == -1 and f"nb = {nb + 1} is not the {nb} blocks of these rows" in lib.colate_last_error().decode()
    assert call(nb - 1) == -1 and f"nb = {nb - 1} is not the {nb} blocks" in lib.colate_last_error().decode()
    assert call(nb, None) == -1 and "NULL pointer" in lib.colate_last_error().decode()
    assert call(nb, counts.ctypes.data, None) == -1 and "NULL pointer" in lib.colate_last_error().decode()
    assert (counts == -7).all()
    assert call(nb) == 0 and (counts.reshape(-1)[:3 * nb * 33] >= 0).all() and (counts.reshape(-1)[3 * nb * 33:] == -7).all()


# ------------------------------------------------------------------ 7. the command line
COMMON = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--age_profile", jl.BINS]


def staged(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    return meta


def modelled_files(nbpb):
    case, meta, _, _ = jl.fixture_case()
    nb = int(jl.blocks_model(case["row_off"], case["rows"]["pos"], nbpb)[-1])
    counts = xl.dense(xl.model(case, EPOCHS[23], nbpb), (14, nb, 23, 3))
    printed = ["%g" % x for x in colate_amd.epochs_from_bins(jl.BINS)[0]]
    return xl.files([" ".join(t["names"]) for t in meta["triples"]], printed, counts.tolist())


def test_cli_files_are_the_models_and_the_forms_agree(tmp_path):
    staged(tmp_path)
    jk = ["--jackknife", "--block_bases", "5000000"]
    runs = {"N": (tl.HOST, []), "S1": (tl.HOST, jk + ["--seed", "1"]), "S2": (tl.HOST, jk + ["--seed", "77"]), "D": (tl.HOST, ["--jackknife"]),
            "K": (tl.CURSORS, jk), "KN": (tl.CURSORS, [])}
    case = jl.fixture_case()[0]
    for out, (env, more) in runs.items():
        r = tl.run_cli(tmp_path, COMMON + ["--expected", "-o", out] + more, env)
        assert r.returncode == 0, (out, r.stderr[-800:])
        nb = int(colate_amd.topo_blocks(case["row_off"], case["rows"], 5_000_000 if "--block_bases" in more else 30_000_000)[-1])
        assert (f"5 samples staged, 14 triples expected in {nb} blocks on the host\n" in r.stderr) == (env is tl.HOST), (out, r.stderr[-800:])
        assert "on the device" not in r.stderr and "drawn on the host\n" not in r.stderr and "profiled" not in r.stderr
        # exactly its own files: nothing sampled
        want_files = [out + ".expected.txt"] + ([out + ".expected.jackknife.txt"] if "--jackknife" in more else [])
        assert sorted(f.name for f in tmp_path.glob(out + "[._]*")) == sorted(want_files), out
    table, jackknifed = modelled_files(5_000_000)
    assert len(table.splitlines()) == 14 * 23 and len(jackknifed.splitlines()) == 14 * 24 and " all " in jackknifed
    for out in runs:
        assert (tmp_path / f"{out}.expected.txt").read_text() == table, out  # (whatever the blocks, the seed and the form)
    for out in ("S1", "S2", "K"):
        assert (tmp_path / f"{out}.expected.jackknife.txt").read_text() == jackknifed, out
    default = (tmp_path / "D.expected.jackknife.txt").read_text()
    assert default == modelled_files(30_000_000)[1] and default != jackknifed
    fractional = [line for line in table.splitlines() if not line.split(" ")[4].endswith(".000000")]
    assert len(fractional) > 50  # the fixture's read counts are not pseudo-haploid: the expectation is no integer
    zs = [line.split(" ")[10] for line in jackknifed.splitlines() if line.split(" ")[3] == "all"]
    assert len(zs) == 14 and all(z != "NA" for z in zs)


def test_cli_refusals_come_before_any_file(tmp_path):
    meta = staged(tmp_path)

    def run(args, env=tl.HOST):
        r = tl.run_cli(tmp_path, args + ["-o", "X"], env)
        assert r.returncode == 1 and not list(tmp_path.glob("X*")), (r.returncode, r.stderr[-500:], list(tmp_path.glob("X*")))
        return r.stderr

    assert "Error: --profile_only does not go with --expected" in run(COMMON + ["--expected", "--profile_only"])
    assert "Error: --expected needs --age_profile x,y,stepsize." in run(COMMON[:-2] + ["--expected"])
    t = meta["triples"][0]
    single = ["--mut", "P", "-i", t["cond"], "--target_tmp", t["target"], "--reference_tmp", t["reference"], "--chr", "chr.txt"]
    assert "--expected needs --mode count_topo --samples" in run(single + ["--expected"], None)
