"""`Colate --mode compare_tmp` without a device: the command line against the reference's own files
(tests/golden/compare_tmp, make_golden_compare.py) on the cursor path and on the host twin, colate_compare_samples_host
against the numpy model of the contract and against the cursor walk, and the refusals by name."""
import numpy as np
import pytest

import colate_amd
import compare_tmp_lib as cl


# ------------------------------------------------------------------ the reference's files
def test_single_runs_write_the_references_files(tmp_path):
    meta = cl.stage(tmp_path)
    for p in meta["pairs"]:
        r = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", p["target"], "--reference_tmp", p["reference"], "--chr", "chr.txt", "-o", "mine.txt"])
        assert r.returncode == 0, r.stderr[-800:]
        assert "compared on the" not in r.stderr  # the cursor walk: nothing staged, no device asked for
        assert (tmp_path / "mine.txt").read_bytes() == (tmp_path / p["output"]).read_bytes(), p["names"]


def test_both_orders_of_a_pair_are_in_the_fixture(tmp_path):
    meta = cl.stage(tmp_path)
    names = [tuple(p["names"]) for p in meta["pairs"]]
    assert ("a", "c") in names and ("c", "a") in names
    assert (tmp_path / "expected_a_c.txt").read_bytes() == (tmp_path / "expected_c_a.txt").read_bytes()


def test_no_chr_single_run_is_the_references(tmp_path):
    meta = cl.stage(tmp_path, "nochr")
    r = cl.run_cli(tmp_path, meta["args"][2:-1] + ["mine.txt"])
    assert r.returncode == 0, r.stderr[-800:]
    mine = (tmp_path / "mine.txt").read_bytes()
    assert mine == (tmp_path / "expected.txt").read_bytes() and mine.startswith(b" ")  # the empty name: a line starts with a blank


@pytest.mark.parametrize("env, said", [(cl.HOST, "4 samples staged, 7 pairs compared on the host"), (cl.CURSORS, "through the record cursors")])
def test_samples_on_the_host_write_every_pairs_file_and_the_matrix(env, said, tmp_path):
    meta = cl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    r = cl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "-o", "S"], env)
    assert r.returncode == 0, r.stderr[-800:]
    assert "pairs compared on the host (COLATE_DEVICE_COMPARE=0)" in r.stderr and said in r.stderr, r.stderr[-800:]
    cl.assert_samples_files(tmp_path, meta, "S")


def test_the_seed_changes_no_byte(tmp_path):
    cl.stage(tmp_path)
    out = []
    for seed in (1, 2):
        r = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", "T1.colate.in", "--reference_tmp", "R1.colate.in", "--chr", "chr.txt", "--seed", seed,
                                  "-o", f"seed{seed}.txt"])
        assert r.returncode == 0, r.stderr[-800:]
        out.append((tmp_path / f"seed{seed}.txt").read_bytes())
    assert out[0] == out[1] == (tmp_path / "expected_b_d.txt").read_bytes()


# ------------------------------------------------------------------ the host twin against the model and the cursor walk
@pytest.mark.parametrize("name", sorted(cl.cases()))
def test_twin_equals_the_model(name):
    c = cl.cases()[name]
    got = cl.compare(c, device=False)
    cl.assert_same(got, cl.modelled(name))
    cl.assert_symmetric(c, got)


def test_the_edge_cases_are_what_they_say():
    c = cl.cases()["sizes"]
    assert np.diff(c["row_off"]).tolist() == [1, 63, 64, 65, 0, 256, 257]
    win_off, mm, n = cl.modelled("sizes")
    assert mm.sum() > 50 and (n - mm).sum() > 50
    for ch in range(7):
        lo, hi = int(c["row_off"][ch]), int(c["row_off"][ch + 1])
        w = cl.window_of(c["rows"]["pos"][lo:hi], int(c["first_pos"][ch]), 7)
        W = int(win_off[ch + 1] - win_off[ch])
        if hi - lo >= 63:
            assert (np.bincount(w // 1, minlength=W) == 0).sum() >= 5 + 1  # empty windows inside and behind the rows
            assert max(len(set(w[k:k + 64].tolist())) for k in range(0, hi - lo, 64)) >= 4  # three boundaries in a word
            d = c["rows"]["pos"][lo:hi].astype(np.int64) - int(c["first_pos"][ch])
            assert (d % 7 == 0).any() and (d % 7 == 1).any()
            assert (np.diff(c["rows"]["pos"][lo:hi]) == 0).any()
    assert win_off[5] - win_off[4] == 5 and (n[:, win_off[4]:win_off[5]] == 0).all()  # no searched row: W_c windows of zeros
    assert (c["idx"]["prev_bp"] == -2).any() and ((c["idx"]["DAF"] | c["idx"]["AAF"]) == 0).any()
    assert n[:, win_off[1]].min() >= 0 and c["rows"]["pos"][0] > c["rows"]["pos"][1]
    assert cl.modelled("many_windows")[0][-1] > 3000


def test_twin_equals_the_cursor_walk_and_the_model_on_files(tmp_path):
    c = cl.write_file_case(str(tmp_path))
    want = cl.model(c)
    cl.assert_same(cl.compare(c, device=False), want)
    assert want[2].sum() > 300 and want[1].sum() > 50 and (want[2] == 0).any()
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt"]
    for out, env, said in (("H", cl.HOST, "3 samples staged, 6 pairs compared on the host"), ("K", cl.CURSORS, "through the record cursors")):
        r = cl.run_cli(tmp_path, common + ["-o", out], env)
        assert r.returncode == 0 and said in r.stderr, r.stderr[-800:]
    for j, (t, r) in enumerate(cl.ALL_PAIRS):
        twin, cursors = (tmp_path / f"H_s{t}_s{r}.txt").read_bytes(), (tmp_path / f"K_s{t}_s{r}.txt").read_bytes()
        assert twin == cursors, (t, r)
        mm, n = cl.read_windows(tmp_path / f"K_s{t}_s{r}.txt")
        assert (mm == want[1][j]).all() and (n == want[2][j]).all(), (t, r)
    r = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", "s0.colate.in", "--reference_tmp", "s2.colate.in", "--chr", "chr.txt", "-o", "one.txt"])
    assert r.returncode == 0 and (tmp_path / "one.txt").read_bytes() == (tmp_path / "K_s0_s2.txt").read_bytes()


def test_rows_that_descend_take_the_cursors(tmp_path):
    """a .mut file whose raw rows descend once: the windows follow the reference's loop row by row, on the cursors"""
    cl.write_file_case(str(tmp_path))
    lines = (tmp_path / "P_chr2.mut").read_text().split("\n")
    lines[40], lines[200] = lines[200], lines[40]
    (tmp_path / "P_chr2.mut").write_text("\n".join(lines))
    r = cl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "-o", "D"], cl.HOST)
    assert r.returncode == 0 and "through the record cursors" in r.stderr, r.stderr[-800:]
    one = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", "s1.colate.in", "--reference_tmp", "s0.colate.in", "--chr", "chr.txt", "-o", "one.txt"])
    assert one.returncode == 0 and (tmp_path / "one.txt").read_bytes() == (tmp_path / "D_s1_s0.txt").read_bytes()


# ------------------------------------------------------------------ refusals
def test_refusals_of_the_call_name_their_argument():
    c = cl.cases()["sizes"]

    def refused(what, **change):
        d = dict(c, **change)
        with pytest.raises(colate_amd.ColateError, match=what):
            cl.compare(d, device=False, cap=d.get("cap"))

    refused("window = 0 must be at least 1", window=0)
    ro = c["row_off"].copy()
    ro[2], ro[3] = ro[3], ro[2]
    refused("row_off decreases at chromosome 2", row_off=ro)
    pr = c["pairs"].copy()
    pr[3]["reference"] = 3
    refused("pair 3: sample id out of range", pairs=pr)
    pr = c["pairs"].copy()
    pr[1]["target_mask"] = 0
    refused("pair 1: compare_tmp takes no masks", pairs=pr)
    first = c["first_pos"].copy()
    first[2] = c["rows"]["pos"][c["row_off"][2]] + 1
    refused("chromosome 2: first_pos", first_pos=first)
    last = c["last_pos"].copy()
    last[6] = c["rows"]["pos"][-1] - 1
    refused("chromosome 6: last_pos", last_pos=last)
    rows = c["rows"].copy()
    rows["pos"][int(c["row_off"][3]) + 2] = 0
    refused("chromosome 3, row 2: position 0 is negative or below the row in front", rows=rows)
    refused("needed: ", cap=6 * int(cl.modelled("sizes")[0][-1]) - 1)
    lib = colate_amd.api.lib
    assert lib.colate_compare_samples_host(1, None, None, 1, None, 1, None, None, None, 7, 0, None, None, None) == -1
    assert "NULL pointer" in lib.colate_last_error().decode()


def test_refusals_of_the_command_line_name_their_line_or_option(tmp_path):
    cl.stage(tmp_path)
    ok = ["a T.colate.in", "c R.colate.in"]

    def run(lines, more=()):
        (tmp_path / "s.txt").write_text("\n".join(lines) + "\n")
        r = cl.run_cli(tmp_path, ["--samples", "s.txt", "--mut", "P", "--chr", "chr.txt", "-o", "X"] + list(more), cl.HOST)
        assert r.returncode == 1 and not list(tmp_path.glob("X*")), r.stderr[-500:]  # nothing is written
        return r.stderr

    assert "s.txt, line 2: mask= is not supported by --mode compare_tmp" in run(["a T.colate.in", "c R.colate.in mask=m"])
    assert "s.txt, line 1: unknown key 'age'" in run(["a T.colate.in age=100", "c R.colate.in"])
    for o, v in (("pairs", "x"), ("target_tmp", "T.colate.in"), ("reference_tmp", "R.colate.in"), ("target_mask", "m"), ("reference_mask", "m"),
                 ("target_age", "1"), ("reference_age", "1"), ("bins", "3,7,0.2"), ("coal", "x.coal"), ("num_bootstraps", "2"), ("ranks", "2"),
                 ("devices", "2")):
        assert f"--{o} cannot be combined with --mode compare_tmp --samples" in run(ok, ["--" + o, v]), o
    assert "cannot open missing.colate.in" in run(["a T.colate.in", "c missing.colate.in"])
    r = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", "T.colate.in", "--reference_tmp", "nope.colate.in", "--chr", "chr.txt", "-o", "X"])
    assert r.returncode == 1 and "cannot open nope.colate.in" in r.stderr and not list(tmp_path.glob("X*"))
    import gzip
    head = gzip.open(tmp_path / "P_chr1.mut.gz", "rt").readline()
    for ch in "123":
        (tmp_path / f"E_chr{ch}.mut").write_text(head)
    r = cl.run_cli(tmp_path, ["--mut", "E", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--chr", "chr.txt", "-o", "X"])
    assert r.returncode == 1 and "E_chr1.mut has no rows" in r.stderr and not list(tmp_path.glob("X*")), r.stderr[-500:]
