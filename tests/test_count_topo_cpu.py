"""`Colate --mode count_topo` without a device: the command line against the reference's own files (tests/golden/count_topo,
make_golden_topo.py) on the cursor path and on the host twin, colate_topo_samples_host against the numpy model of the contract
and against the cursor walk, and the refusals by name."""
import numpy as np
import pytest

import colate_amd
import count_topo_lib as tl


# ------------------------------------------------------------------ the reference's files
def test_single_runs_write_the_references_files(tmp_path):
    meta = tl.stage(tmp_path)
    for p in meta["triples"]:
        r = tl.run_cli(tmp_path, ["--mut", "P", "-i", p["cond"], "--target_tmp", p["target"], "--reference_tmp", p["reference"], "--chr", "chr.txt",
                                  "--seed", meta["seed"], "-o", "mine.txt"])
        assert r.returncode == 0, r.stderr[-800:]
        assert "drawn on the" not in r.stderr  # the cursor walk: nothing staged, no device asked for
        assert (tmp_path / "mine.txt").read_bytes() == (tmp_path / p["output"]).read_bytes(), p["names"]


def test_the_fixture_holds_what_the_contract_turns_on(tmp_path):
    meta = tl.stage(tmp_path)
    names = [tuple(p["names"]) for p in meta["triples"]]
    assert ("e", "b", "c") in names and ("e", "c", "b") in names  # both orders of a (target, reference) pair
    flip = {1: -1, -1: 1}
    a, b = tl.read_lines(tmp_path / "expected_e_b_c.txt"), tl.read_lines(tmp_path / "expected_e_c_b.txt")
    assert a != [(n, pos, flip[s], -v) for n, pos, s, v in b]  # the draws are not symmetric: d1 belongs to the target
    for p in meta["triples"]:
        assert p["plus"] > 10 and p["minus"] > 10, p["names"]
    ages = [line.split(" ")[2:4] for p in meta["triples"] for line in (tmp_path / p["output"]).read_text().splitlines()]
    assert any(x == y for x, y in ages)  # a printed row with age_begin == age_end: `<=` in the row filter


def test_the_seed_decides_the_file(tmp_path):
    tl.stage(tmp_path)
    out = []
    for seed in (5, 6):
        r = tl.run_cli(tmp_path, ["--mut", "P", "-i", "T2.colate.in", "--target_tmp", "T1.colate.in", "--reference_tmp", "R1.colate.in", "--chr",
                                  "chr.txt", "--seed", seed, "-o", f"seed{seed}.txt"])
        assert r.returncode == 0, r.stderr[-800:]
        out.append((tmp_path / f"seed{seed}.txt").read_bytes())
    assert out[0] == (tmp_path / "expected_e_b_d.txt").read_bytes() and out[1] != out[0]


def test_no_chr_single_run_is_the_references(tmp_path):
    meta = tl.stage(tmp_path, "nochr")
    r = tl.run_cli(tmp_path, meta["args"][2:-1] + ["mine.txt"])
    assert r.returncode == 0, r.stderr[-800:]
    mine = (tmp_path / "mine.txt").read_bytes()
    assert mine == (tmp_path / "expected.txt").read_bytes() and mine.startswith(b" ")  # the empty name: a line starts with a blank
    r = tl.run_cli(tmp_path, meta["args"][2:-1] + ["twin.txt"], {"COLATE_DEVICE_TOPO": "1"})  # an empty name cannot be indexed
    assert r.returncode == 0 and "through the record cursors" in r.stderr, r.stderr[-800:]
    assert (tmp_path / "twin.txt").read_bytes() == mine


@pytest.mark.parametrize("env, said", [(tl.HOST, "5 samples staged, 14 triples drawn on the host"), (tl.CURSORS, "through the record cursors")])
def test_samples_on_the_host_write_every_triples_file_and_the_totals(env, said, tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    r = tl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", meta["seed"], "-o", "S"], env)
    assert r.returncode == 0, r.stderr[-800:]
    assert "triples drawn on the host (COLATE_DEVICE_TOPO=0)" in r.stderr and said in r.stderr, r.stderr[-800:]
    tl.assert_samples_files(tmp_path, meta, "S")


# ------------------------------------------------------------------ the host twin against the model and the cursor walk
@pytest.mark.parametrize("name", sorted(tl.cases()))
def test_twin_equals_the_model_on_the_edge_cases(name):
    got = tl.topo(tl.cases()[name], device=False)
    tl.assert_same(got, tl.modelled(name))
    tl.assert_edges(name, got)


def test_the_edge_cases_are_what_they_say():
    c = tl.cases()["sizes"]
    assert np.diff(c["row_off"]).tolist() == [0, 1, 63, 64, 65, 200]
    assert np.diff(tl.cases()["tiles"]["row_off"]).tolist() == [tl.TILE - 1, tl.TILE, tl.TILE + 1] and tl.TILE == 4096
    for name in tl.cases():
        c = tl.cases()[name]
        _, plus, minus, draws = tl.modelled(name)
        word_off = tl.modelled(name)[0]
        last = int(c["row_off"][-2])
        q = plus[tl.SPARSE_Q] | minus[tl.SPARSE_Q]  # the two qualifying rows sit on bit 63 and on bit 0 (whatever their sign)
        assert (q & ~np.uint64((1 << 63) | 1) == 0).all()
        hit = (c["idx"]["DAF"] | c["idx"]["AAF"]) != 0
        assert hit[tl.SPARSE].nonzero()[0].tolist() == [last + 127, last + 192] and not hit[tl.EMPTY].any()
        assert (c["cond_idx"]["DAF"][tl.EMPTY] > 0).all()
        assert word_off[-1] == ((np.diff(c["row_off"]) + 63) // 64).sum()
        # the ranks run on across the chromosomes: the rows in front of the last chromosome have qualified before it
        assert draws[0] > 64 and (hit[tl.RANDOM1] & hit[tl.RANDOM2])[:last].sum() > 32


def test_a_stream_one_uniform_short_is_refused_with_the_needed_length():
    c = tl.cases()["sizes"]
    n = c["rows"].size
    short = dict(c, uniforms=c["uniforms"][:-1])
    with pytest.raises(colate_amd.ColateError, match=f"needed: {2 * n}"):
        tl.topo(short, device=False)
    with pytest.raises(ValueError, match=f"needed: {2 * n}"):
        tl.model(short)


def test_twin_equals_the_cursor_walk_and_the_model_on_files(tmp_path):
    c = tl.write_file_case(str(tmp_path))
    seed = 9
    c["uniforms"] = tl.mt_uniforms(seed, 2 * c["rows"].size)
    want = tl.model(c)
    got = tl.topo(c, device=False)
    tl.assert_same(got, want)
    assert want[3].min() > 20 and want[1].any(axis=1).all() and want[2].any(axis=1).all()
    # a conditioning record that is not the row's: a sample that ended before the chromosome's last rows qualifies there
    unmatched = (c["cond_idx"]["DAF"] > 0) & ((c["idx"]["DAF"] | c["idx"]["AAF"]) == 0)
    assert unmatched[1].any() and unmatched[3].any()
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", seed]
    for out, env, said in (("H", tl.HOST, "4 samples staged, 24 triples drawn on the host"), ("K", tl.CURSORS, "through the record cursors")):
        r = tl.run_cli(tmp_path, common + ["-o", out], env)
        assert r.returncode == 0 and said in r.stderr, r.stderr[-800:]
    totals = (tmp_path / "H.triples.txt").read_text().splitlines()
    assert totals == (tmp_path / "K.triples.txt").read_text().splitlines()
    printed_unmatched = 0
    for p, t in enumerate(c["triples"]):
        name = f"s{t['cond']}_s{t['target']}_s{t['reference']}"
        twin, cursors = (tmp_path / f"H_{name}.txt").read_bytes(), (tmp_path / f"K_{name}.txt").read_bytes()
        assert twin == cursors and len(twin) > 50, name
        mine = tl.lines_of(c, got, p)
        # (the value is printed as the stream's default does it: six significant digits)
        assert [(n, pos, s, float("%g" % (s * daf / N))) for n, pos, s, daf, N in mine] == tl.read_lines(tmp_path / f"K_{name}.txt"), name
        plus, minus = sum(x[2] > 0 for x in mine), sum(x[2] < 0 for x in mine)
        assert totals[p] == f"{name.replace('_', ' ')} {plus} {minus} {want[3][p]}", totals[p]
    for g in np.nonzero(unmatched[1])[0]:
        printed_unmatched += any(tl.bit(got[1] | got[2], c, p, int(g)) for p, t in enumerate(c["triples"]) if t["cond"] == 1)
    assert printed_unmatched > 0
    r = tl.run_cli(tmp_path, ["--mut", "P", "-i", "s1.colate.in", "--target_tmp", "s0.colate.in", "--reference_tmp", "s2.colate.in", "--chr", "chr.txt",
                              "--seed", seed, "-o", "one.txt"])
    assert r.returncode == 0 and (tmp_path / "one.txt").read_bytes() == (tmp_path / "K_s1_s0_s2.txt").read_bytes()


def test_counts_beyond_16_bits_and_rows_that_descend_take_the_cursors(tmp_path):
    tl.write_file_case(str(tmp_path), big_counts=True)  # sample 2 carries counts up to 120 000
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", 3]
    r = tl.run_cli(tmp_path, common + ["-o", "B"], tl.HOST)
    assert r.returncode == 0 and "through the record cursors" in r.stderr, r.stderr[-800:]
    lines = (tmp_path / "P_chr2.mut").read_text().split("\n")
    lines[40], lines[200] = lines[200], lines[40]
    (tmp_path / "P_chr2.mut").write_text("\n".join(lines))
    r = tl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", 3, "-o", "D"], tl.HOST)
    assert r.returncode == 0 and "through the record cursors" in r.stderr, r.stderr[-800:]
    one = tl.run_cli(tmp_path, ["--mut", "P", "-i", "s3.colate.in", "--target_tmp", "s1.colate.in", "--reference_tmp", "s0.colate.in", "--chr", "chr.txt",
                                "--seed", 3, "-o", "one.txt"])
    assert one.returncode == 0 and (tmp_path / "one.txt").read_bytes() == (tmp_path / "D_s3_s1_s0.txt").read_bytes()


# ------------------------------------------------------------------ refusals
def test_refusals_of_the_call_name_their_argument():
    c = tl.cases()["sizes"]

    def refused(what, **change):
        d = dict(c, **change)
        with pytest.raises(colate_amd.ColateError, match=what):
            tl.topo(d, device=False, cap=d.get("cap"))

    ro = c["row_off"].copy()
    ro[2], ro[3] = ro[3], ro[2]
    refused("row_off decreases at chromosome 2", row_off=ro)
    for role in ("cond", "target", "reference"):
        tr = c["triples"].copy()
        tr[3][role] = 7
        refused("triple 3: sample id out of range", triples=tr)
    rows = c["rows"].copy()
    rows["pos"][int(c["row_off"][4]) + 2] = 0
    refused("chromosome 4, row 2: position 0 is negative or below the row in front", rows=rows)
    refused("needed: ", cap=len(tl.TRIPLES) * int(tl.modelled("sizes")[0][-1]) - 1)
    lib = colate_amd.api.lib
    assert lib.colate_topo_samples_host(1, None, None, 1, None, None, 1, None, 0, None, 0, None, None, None, None) == -1
    assert "NULL pointer" in lib.colate_last_error().decode()
    with pytest.raises(ValueError, match="cond_idx must be"):
        colate_amd.topo_samples(c["row_off"], c["rows"], c["idx"], c["cond_idx"][:3], c["triples"], c["uniforms"], device=False)


def test_refusals_of_the_command_line_name_their_line_or_option(tmp_path):
    tl.stage(tmp_path)
    ok = ["a T.colate.in", "b T1.colate.in", "c R.colate.in"]

    def run(lines, more=()):
        (tmp_path / "s.txt").write_text("\n".join(lines) + "\n")
        r = tl.run_cli(tmp_path, ["--samples", "s.txt", "--mut", "P", "--chr", "chr.txt", "-o", "X"] + list(more), tl.HOST)
        assert r.returncode == 1 and not list(tmp_path.glob("X*")), r.stderr[-500:]  # nothing is written
        return r.stderr

    assert "s.txt, line 2: mask= is not supported by --mode count_topo" in run(["a T.colate.in", "b T1.colate.in mask=m", "c R.colate.in"])
    assert "s.txt, line 1: unknown key 'age'" in run(["a T.colate.in age=100", "b T1.colate.in", "c R.colate.in"])
    assert "s.txt, line 3: unknown role 'both' (known: cond, target, reference)" in run(ok[:2] + ["c R.colate.in role=cond,both"])
    assert "s.txt, line 1: the role 'cond' is given twice" in run(["a T.colate.in role=cond,cond"] + ok[1:])
    assert "the list names no cond sample" in run([x + " role=target,reference" for x in ok])
    assert "the list names no reference sample" in run([x + " role=cond,target" for x in ok])
    assert "no triple of a cond, a target and a reference on three different lines" in run(ok[:2])
    for o, v in (("input", "T.colate.in"), ("pairs", "x"), ("target_tmp", "T.colate.in"), ("reference_tmp", "R.colate.in"), ("target_mask", "m"),
                 ("reference_mask", "m"), ("target_age", "1"), ("reference_age", "1"), ("bins", "3,7,0.2"), ("coal", "x.coal"), ("num_bootstraps", "2"),
                 ("ranks", "2"), ("devices", "2")):
        assert f"--{o} cannot be combined with --mode count_topo --samples" in run(ok, ["--" + o, v]), o
    assert "Failed to open missing.colate.in" in run(ok[:2] + ["c missing.colate.in"])
    single = ["--mut", "P", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--chr", "chr.txt", "-o", "X"]
    r = tl.run_cli(tmp_path, single + ["-i", "nope.colate.in"])
    assert r.returncode == 1 and "Failed to open nope.colate.in" in r.stderr and not list(tmp_path.glob("X*"))
    r = tl.run_cli(tmp_path, single)  # no --input: the reference's two lines and the help
    assert r.returncode == 0 and not list(tmp_path.glob("X*"))
    assert r.stdout.startswith("Not enough arguments supplied.\nNeeded: target_tmp, reference_tmp, input, mut, output. Optional: chr.\n")
    assert r.stdout.rstrip().endswith("Compare tmp.")


def test_every_other_mode_still_refuses_the_cond_role(tmp_path):
    import compare_tmp_lib as cl
    cl.stage(tmp_path)
    (tmp_path / "s.txt").write_text("a T.colate.in role=cond\nc R.colate.in\n")
    r = cl.run_cli(tmp_path, ["--samples", "s.txt", "--mut", "P", "--chr", "chr.txt", "-o", "X"], cl.HOST)
    assert r.returncode == 1 and "s.txt, line 1: unknown role 'cond' (known: target, reference)" in r.stderr, r.stderr[-500:]
    import subprocess
    r = subprocess.run([cl.il.CLI, "--mode", "no_such_mode"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--mode count_topo" in r.stdout and "print_tmp stay with the reference build" in r.stdout
