"""colate_fill_samples_host (the host twin of the table fill over walk indices) and `Colate --mode mut --samples` on the host
path: no GPU needed.  The device's side of the same cases is tests/test_gpu_fill_samples.py."""
import numpy as np
import pytest

import colate_amd
import fill_samples_lib as fl
import interval_walk_lib as wl

NAMES = sorted(fl.cases())


@pytest.mark.parametrize("name", NAMES)
def test_twin_walks_as_the_model_and_reproduces(name):
    """nb and used are the walk model's; a second call gives the same bits; a pair's generator has given out 200 words per
    used row unless a draw was repeated"""
    c = fl.cases()[name]
    got = fl.twin(name)
    if name in wl.cases():
        rec_off, nb, _, _ = wl.modelled(name)
    else:
        rec_off, nb, _, _ = wl.model(c)
    assert np.array_equal(got["nb"], nb) and np.array_equal(got["used"], np.diff(rec_off))
    fl.assert_same_fill(fl.fill(c, device=False), got)
    assert (got["handed_back"] == 0).all()
    want_near = fl.HANDED_BACK.get(name, [0] * len(nb))
    # (the condition that keeps the GPU tests from passing through the hand-back: other seeds if a case trips it)
    assert got["near_band"].tolist() == want_near, (name, got["near_band"])
    clean = np.array(want_near) == 0
    assert np.array_equal(got["words"][clean], 200 * got["used"][clean].astype(np.uint64))
    assert (got["words"][~clean] > 200 * got["used"][~clean].astype(np.uint64)).all()
    for p, t in enumerate(got["tables"]):
        assert t.shape == (nb[p], 4, fl.A) and np.isfinite(t).all() and (t >= 0).all()


def test_twin_tables_add_up():
    """what is independent of the draws: a non-F record spreads 100 hundredths of its weights, an F record whose ages stay
    within the grid 100 hundredths of its not-shared weight and one un-divided pair into row 0"""
    c = fl.cases()["frow_bins"]
    got = fl.twin("frow_bins")
    _, _, recs, block = wl.model(c)  # (the interval record carries the un-divided weights)
    for b in range(2):
        sel = block == b
        t = got["tables"][0][b]
        assert t[0].sum() == 0.0  # F records add nothing to the shared table
        assert np.isclose(t[1].sum(), recs["w_ns"][sel].sum(), rtol=1e-12)
        assert np.isclose(t[2].sum(), recs["w_sh"][sel].sum(), rtol=1e-12) and np.isclose(t[3].sum(), recs["w_ns"][sel].sum(), rtol=1e-12)
    assert (got["tables"][0][0][2] != 0).sum() == 1 and (got["tables"][0][1][2] != 0).sum() == 64  # one bin; 64 different bins
    # the block of the record that ends beyond the grid: 64 of its 65 F records reach row 0
    rec_off, _, recs, block = wl.model(fl.cases()["frow_sizes"])
    recs, block = recs[: rec_off[1]], block[: rec_off[1]]
    f_rows = np.flatnonzero((block == 2) & (recs["begin"] <= 0))
    assert f_rows.size == 65 and recs["end"][f_rows[-1]] > 1e7
    row0 = fl.twin("frow_sizes")["tables"][0][2][3]
    assert np.isclose(row0.sum(), recs["w_ns"][f_rows[:-1]].sum(), rtol=1e-12)
    assert (fl.twin("frow_sizes")["tables"][0][4][2:] == 0).all()  # the block without an F record


def test_seed_moves_the_tables_and_nothing_else():
    c = fl.cases()["sizes"]
    a, b = fl.fill(c, device=False, seed=1), fl.fill(c, device=False, seed=2)
    assert np.array_equal(a["nb"], b["nb"]) and np.array_equal(a["used"], b["used"])
    assert any((x != y).any() for x, y in zip(a["tables"], b["tables"]))
    for x, y in zip(a["tables"], b["tables"]):  # row 0 of the F tables takes no draw
        assert np.array_equal(x[:, 2:], y[:, 2:])


def test_refusals():
    c = fl.cases()["one_row"]
    with pytest.raises(colate_amd.ColateError, match="185"):
        fl.fill(c, device=False, A=184)
    with pytest.raises(colate_amd.ColateError, match="185"):
        fl.fill(c, device=False, A=186)
    bad = dict(c, pairs=wl.make_pairs([(0, 3)]))
    with pytest.raises(colate_amd.ColateError, match="sample id out of range"):
        fl.fill(bad, device=False)
    with pytest.raises(colate_amd.ColateError, match="num_bases_per_block"):
        fl.fill(dict(c, nbpb=0), device=False)
    rows = c["rows"].copy()
    rows["pos"][0] = -4
    with pytest.raises(colate_amd.ColateError, match="negative"):
        fl.fill(dict(c, rows=rows), device=False)
    with pytest.raises(colate_amd.ColateError, match="needed: 3"):  # room for fewer blocks than the pairs have
        fl.fill(c, device=False, cap_blocks=2)


# ------------------------------------------------------------------ the command line, host path
@pytest.mark.parametrize("fixture", sorted(fl.FIXTURES))
def test_samples_counts_are_those_of_pairs(fixture, tmp_path):
    """`--samples --counts_only` writes, for every pair of the list, the .counts bytes `--pairs --counts_only` writes for the
    expanded list (ages, masks and outputs included); the fixture's pairs all walk through indices"""
    stage, lists = fl.FIXTURES[fixture]
    meta = stage(str(tmp_path))
    for k, (samples, _) in enumerate(lists):
        rs, rp, names = fl.run_both(tmp_path, meta["common_args"], samples, k, ["--counts_only"])
        fl.assert_all_indexed(rp, len(names))
        assert rs.returncode == 0, rs.stderr[-800:]
        assert "pairs walked and filled through the engine of --pairs (" in rs.stderr
        for i, name in enumerate(names):
            assert f"Pair {i + 1} / {len(names)}: " in rs.stderr
            mine, theirs = (tmp_path / f"s{k}_{name}.counts").read_bytes(), (tmp_path / f"e{k}_{name}.counts").read_bytes()
            assert len(mine) > 1000 and mine == theirs, name


LIST_ERRORS = [
    (["a T.colate.in", "b R.colate.in age=abc"], 2, "the age 'abc' is not a number"),
    (["a T.colate.in age=-5", "b R.colate.in"], 1, "the age '-5' is negative"),
    (["a T.colate.in age=nan", "b R.colate.in"], 1, "is not a number"),
    (["a T.colate.in", "", "b R.colate.in age=1 age=2"], 3, "the key 'age' is given twice"),
    (["a T.colate.in age=", "b R.colate.in"], 1, "the key 'age' has no value"),
    (["a T.colate.in", "b R.colate.in 500"], 2, "'500' is no key=value token"),
    (["a T.colate.in", "a R.colate.in"], 2, "the NAME 'a' is given twice (first on line 1)"),
    (["a T.colate.in", "b/c R.colate.in"], 2, "contains '/'"),
    (["a T.colate.in", "mask=TM R.colate.in"], 2, "the sample's NAME is missing or empty"),
    (["a T.colate.in", "b"], 2, "expected `NAME FILE.colate.in"),
    (["a T.colate.in", "b R.colate.in depth=3"], 2, "unknown key 'depth' (known: mask, role, age)"),
    (["a T.colate.in", "b R.colate.in role=both"], 2, "unknown role 'both'"),
    (["a T.colate.in role=target role=target", "b R.colate.in"], 1, "the key 'role' is given twice"),
    (["a T.colate.in mask=", "b R.colate.in"], 1, "the key 'mask' has no value"),
]


def test_list_errors_name_their_line_and_write_nothing(tmp_path):
    meta = fl.gl.l3_pairs_stage(str(tmp_path))
    before = sorted(p.name for p in tmp_path.iterdir())
    for lines, line_no, what in LIST_ERRORS:
        (tmp_path / "bad.txt").write_text("\n".join(lines) + "\n")
        r = fl.run_cli(tmp_path, meta["common_args"] + ["--samples", "bad.txt", "-o", "x", "--counts_only"])
        assert r.returncode == 1, (lines, r.stderr[-300:])
        assert f"bad.txt, line {line_no}: " in r.stderr and what in r.stderr, (lines, r.stderr[-300:])
    for lines, what in ((["a T.colate.in role=target", "b R.colate.in role=target"], "the list names no reference sample"),
                        (["a T.colate.in"], "no pair of a target and a reference on different lines")):
        (tmp_path / "bad.txt").write_text("\n".join(lines) + "\n")
        r = fl.run_cli(tmp_path, meta["common_args"] + ["--samples", "bad.txt", "-o", "x", "--counts_only"])
        assert r.returncode == 1 and what in r.stderr, r.stderr[-300:]
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(before + ["bad.txt"])


def test_refused_options_and_mut_interval_keeps_refusing_ages(tmp_path):
    meta = fl.gl.l3_pairs_stage(str(tmp_path))
    (tmp_path / "s.txt").write_text("a T.colate.in\nb R.colate.in age=500\n")
    base = meta["common_args"] + ["--samples", "s.txt", "-o", "x", "--counts_only"]
    for o, v in (("pairs", "pairs.txt"), ("target_tmp", "T.colate.in"), ("reference_tmp", "R.colate.in"), ("target_mask", "TM"),
                 ("reference_mask", "RM"), ("target_age", "5"), ("reference_age", "5"), ("ranks", "1")):
        r = fl.run_cli(tmp_path, base + [f"--{o}", v])
        assert r.returncode == 1 and f"--{o} cannot be combined with --mode mut --samples" in r.stderr, (o, r.stderr[-300:])
    r = fl.run_cli(tmp_path, ["--samples", "s.txt", "-o", "x"])
    assert r.returncode == 1 and "--samples needs --mut, -o PREFIX and --bins" in r.stderr
    e = dict(fl.os.environ, COLATE_DEVICE_INTERVAL="0")
    r = fl.subprocess.run([fl.il.CLI, "--mode", "mut_interval", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--samples", "s.txt",
                           "-o", "y"], cwd=str(tmp_path), capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 1 and "s.txt, line 2: unknown key 'age' (known: mask, role)" in r.stderr, r.stderr[-300:]
    assert not list(tmp_path.glob("x*")) and not list(tmp_path.glob("y*"))
