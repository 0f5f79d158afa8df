"""The pair walk over per-sample walk indices on the host: colate_interval_walk_host against the walk contract restated as a
Python loop (interval_walk_lib.model) in every byte, colate_interval_fit_samples_host against colate_interval_fit_groups_host
on those records with weights drawn from the same seed, every refusal by name, and `Colate --mode mut_interval --samples`
with the host twins against `--pairs` on the expanded list and against single runs."""
import numpy as np
import pytest

import colate_amd
import interval_cells_lib as il
import interval_groups_lib as gl
import interval_walk_lib as wl

CASES = list(wl.cases())


def test_the_cases_cover_what_they_are_built_for():
    W, c = wl.W, wl.cases()
    assert np.diff(c["sizes"]["row_off"]).tolist() == [1, W - 1, W, W + 1, 3 * W + 5]
    prs = [tuple(int(p[k]) for k in ("target", "reference")) for p in c["sizes"]["pairs"]]
    assert len(prs) == 5 and len(set(prs)) == 4 and any(t == r for t, r in prs) and c["sizes"]["idx"].shape[0] == 3
    # the carry: reference-passing rows in the first and the last of four tiles only, used rows on both sides
    rec_off, nb, recs, block = wl.modelled("carry")
    assert np.diff(rec_off).tolist() == [4, 0, 4]
    ref = c["carry"]["idx"][1]["DAF"]
    assert ref[:W].any() and not ref[W:3 * W].any() and ref[3 * W:].any()
    # masks: a whole tile removed, every row removed (no record, one block per chromosome), words ending mid-word
    assert np.diff(wl.modelled("masks")[0])[3] == 0 and wl.modelled("masks")[1][3] == 3
    assert any(n % 64 for n in np.diff(c["masks"]["row_off"]))
    # equal positions on both sides of a tile edge
    pos = c["equal_positions"]["rows"]["pos"]
    assert pos[W - 1] == pos[W] and pos[2 * W - 1] == pos[2 * W]
    # the middle chromosome of three without a used row, an empty block in between, and a block per base
    rec_off, nb, recs, block = wl.modelled("blocks")
    b0 = block[:rec_off[1]]
    assert 2 not in b0 and 3 in b0 and 4 not in b0 and nb[0] == 9  # 4 blocks, 1, 4
    assert c["one_base_blocks"]["nbpb"] == 1 and wl.modelled("one_base_blocks")[1].min() > 50
    # the half-way rounding of the target genotype: 1 of 4 reads is a call of 1 (roundf), 65535 of 65535 one of 2
    r = wl.modelled("counts")[2]
    assert r["w_sh"][0] == 0.5 and r["w_ns"][0] == 1.0 and r["w_sh"][3] == 2.0 * 65535 / 65536 and r["begin"][0] == 0.0


@pytest.mark.parametrize("name", CASES)
def test_host_twin_equals_the_python_loop(name):
    wl.assert_same_walk(wl.walk(wl.cases()[name], device=False), wl.modelled(name))


def test_prev_bp_on_one_below_and_one_above_the_row_in_front():
    """the `<` of the rule, unmasked: row 1 passes as reference iff prev_bp >= pos(row 0); the target likewise against the
    latest row that passed as reference; prev_bp = -2 (no record in front: the cursor cannot have moved) never passes"""
    rows = np.zeros(3, dtype=wl.ROW)
    rows["pos"], rows["age_begin"], rows["age_end"] = [100, 200, 300], 10.0, 20.0
    for d_ref, d_tgt, want in [(0, 0, 3), (-1, 0, 2), (1, 1, 3), (0, -1, 2), (-1, -1, 2)]:
        idx = np.zeros((2, 3), dtype=wl.IDX)
        idx[0]["DAF"] = idx[1]["DAF"] = 1
        idx[1]["prev_bp"] = [50, 100 + d_ref, 200]  # reference
        idx[0]["prev_bp"] = [50, 100 + d_tgt, 200 if d_ref >= 0 else 100]  # target: against row 1, or row 0 where row 1 did not pass
        c = wl.case(np.array([0, 3]), rows, idx, wl.make_pairs([(0, 1)]), 1000)
        got = wl.walk(c, device=False)
        wl.assert_same_walk(got, wl.model(c))
        assert got[0][1] == want, (d_ref, d_tgt, got[0])
    idx[1]["prev_bp"] = [-2, -2, -2]
    c = wl.case(np.array([0, 3]), rows, idx, wl.make_pairs([(0, 1)]), 1000)
    assert wl.walk(c, device=False)[0][1] == 0 and wl.model(c)[0][1] == 0


def test_capacity():
    c = wl.cases()["sizes"]
    total = int(wl.modelled("sizes")[0][-1])
    wl.assert_same_walk(wl.walk(c, device=False, cap=total), wl.modelled("sizes"))
    with pytest.raises(colate_amd.ColateError, match=f"needed: {total}") as e:
        wl.walk(c, device=False, cap=total - 1)
    assert e.value.code == -4  # COLATE_ELIMIT


@pytest.mark.parametrize("name", ["sizes", "masks", "blocks", "counts"])
def test_fit_samples_host_equals_fit_groups_host_on_the_walks_records(name):
    c = wl.cases()[name]
    wl.assert_same_fit(wl.fit_samples(c, device=False), wl.fit_groups_on(wl.modelled(name), device=False))


def test_fit_samples_host_under_small_budgets(monkeypatch):
    """(the budgets shape the device's chunks; the host twin's results do not know them)"""
    c = wl.cases()["blocks"]
    want = wl.fit_groups_on(wl.modelled("blocks"), device=False)
    monkeypatch.setenv("COLATE_INTERVAL_GROUPS_CELLS_MB", "1")
    monkeypatch.setenv("COLATE_INTERVAL_WALK_RECS_MB", "0")
    wl.assert_same_fit(wl.fit_samples(c, device=False), want)


# ------------------------------------------------------------------ refusals
def refused(match, **change):
    c = dict(wl.cases()["blocks"], **change)
    for call in (lambda: wl.walk(c, device=False), lambda: wl.fit_samples(c, device=False)):
        with pytest.raises(colate_amd.ColateError, match=match):
            call()


def test_refusals_by_name():
    c = wl.cases()["blocks"]

    def pairs(**kw):
        p = c["pairs"].copy()
        for k, v in kw.items():
            p[k][1] = v
        return p

    refused("sample id out of range", pairs=pairs(target=3))
    refused("sample id out of range", pairs=pairs(reference=-1))
    refused("mask id out of range", pairs=pairs(target_mask=0))
    refused("mask id out of range", pairs=pairs(reference_mask=-2))
    ro = c["row_off"].copy()
    ro[1], ro[2] = ro[2], ro[1]
    refused("row_off decreases at chromosome 1", row_off=ro)
    refused("num_bases_per_block = 0 must be at least 1", nbpb=0)
    rows = c["rows"].copy()
    rows["pos"][-1] = 2 ** 31 - c["nbpb"]
    refused("at or above 2\\^31 - num_bases_per_block", rows=rows)
    rows["pos"][-1] = 2 ** 31 - c["nbpb"] - 1
    wl.assert_same_walk(wl.walk(dict(c, rows=rows), device=False), wl.model(dict(c, rows=rows)))
    rows = c["rows"].copy()
    rows["pos"][5] = rows["pos"][4] - 1
    refused("below the row in front", rows=rows)


def test_null_pointers_and_sizes_are_refused():
    c = wl.cases()["one_row"]
    lib = colate_amd.api.lib
    p = lambda a: a.ctypes.data  # noqa: E731
    rec_off, nb = np.zeros(4, dtype=np.int64), np.zeros(3, dtype=np.int32)
    recs, block = np.zeros(8, dtype=wl.REC), np.zeros(8, dtype=np.int32)
    good = [1, p(c["row_off"]), p(c["rows"]), 3, p(c["idx"]), 0, None, 3, p(c["pairs"]), 100, 8, p(rec_off), p(nb), p(recs), p(block)]
    assert lib.colate_interval_walk_host(*good) == 0
    for k in (1, 2, 4, 8, 11, 12, 13, 14):
        bad = list(good)
        bad[k] = None
        assert lib.colate_interval_walk_host(*bad) < 0 and b"NULL pointer" in lib.colate_last_error(), k
    for k in (0, 3, 7):
        bad = list(good)
        bad[k] = 0
        assert lib.colate_interval_walk_host(*bad) < 0 and b"bad sizes" in lib.colate_last_error(), k
    with pytest.raises(colate_amd.ColateError, match="bad sizes B=0"):
        wl.fit_samples(c, device=False, num_bootstrap=0)


# ------------------------------------------------------------------ the command line
SAMPLES, EXPANDED, run_samples = wl.SAMPLES, wl.EXPANDED, wl.run_samples


@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("samples_cli")
    gl.cli_inputs(d)
    return d


def test_cli_samples_write_the_bytes_of_pairs_and_of_single_runs(cli_dir):
    d = cli_dir
    s = run_samples(d, SAMPLES, "S", device=False)
    assert s.returncode == 0, s.stderr[-2000:]
    assert "4 samples and 1 masks staged, 5 pairs walked on the host" in s.stderr
    gl.write_list(d / "expanded.txt", EXPANDED, prefix="P_")
    p = gl.run_pairs(d, "expanded.txt", device=False)
    assert p.returncode == 0, p.stderr[-2000:]
    for i, pair in enumerate(EXPANDED):
        assert (d / f"S_{pair[2]}.coal").read_bytes() == (d / f"P_{pair[2]}.coal").read_bytes(), pair[2]
        assert gl.pair_lines(s.stderr, i + 1, 5) == gl.pair_lines(p.stderr, i + 1, 5), pair[2]
    one = gl.run_single(d, EXPANDED[3], "single", device=False)
    assert one.returncode == 0, one.stderr[-2000:]
    assert (d / "single.coal").read_bytes() == (d / "S_b_c.coal").read_bytes()
    # the engine's walk on the expanded list, asked for by name: the same bytes after one line
    f = run_samples(d, SAMPLES, "F", device=False, env={"COLATE_DEVICE_INTERVAL_WALK": "0"})
    assert f.returncode == 0 and "pairs walked on the host through the engine (COLATE_DEVICE_INTERVAL_WALK=0)" in f.stderr
    assert "staged" not in f.stderr
    for pair in EXPANDED:
        assert (d / f"F_{pair[2]}.coal").read_bytes() == (d / f"S_{pair[2]}.coal").read_bytes(), pair[2]


def test_cli_samples_without_walk_indices_take_the_pairs_path(cli_dir):
    f = run_samples(cli_dir, SAMPLES, "N", device=False, env={"COLATE_INDEXED_WALK": "0"})
    assert f.returncode == 0 and "pairs walked on the host through the engine (a sample has no walk index)" in f.stderr
    s = run_samples(cli_dir, SAMPLES, "S2", device=False)
    for pair in EXPANDED:
        assert (cli_dir / f"N_{pair[2]}.coal").read_bytes() == (cli_dir / f"S2_{pair[2]}.coal").read_bytes(), pair[2]


@pytest.mark.parametrize("lines, line, what", [
    (["a T.colate.in", "a R.colate.in"], 2, "given twice"),
    (["a T.colate.in", "role=target R.colate.in"], 2, "NAME is missing or empty"),
    (["a T.colate.in", "x/y R.colate.in"], 2, "contains '/'"),
    (["a T.colate.in", "", "b R.colate.in colour=red"], 3, "unknown key 'colour'"),
    (["a T.colate.in", "b R.colate.in 5000"], 2, "ages"),
    (["a T.colate.in role=both", "b R.colate.in"], 1, "unknown role"),
    (["a T.colate.in", "b"], 2, "expected `NAME FILE.colate.in"),
])
def test_cli_list_errors_name_their_line(cli_dir, lines, line, what):
    r = run_samples(cli_dir, lines, "E", device=False)
    assert r.returncode == 1 and f"samples.txt, line {line}: " in r.stderr and what in r.stderr, r.stderr[-800:]
    assert not list(cli_dir.glob("E_*"))


@pytest.mark.parametrize("lines, what", [(["a T.colate.in role=reference", "b R.colate.in role=reference"], "no target"),
                                         (["a T.colate.in role=target"], "no reference")])
def test_cli_a_list_without_a_target_or_a_reference(cli_dir, lines, what):
    r = run_samples(cli_dir, lines, "E", device=False)
    assert r.returncode == 1 and what in r.stderr and not list(cli_dir.glob("E_*")), r.stderr[-800:]


@pytest.mark.parametrize("option", ["pairs", "rows", "target_tmp", "reference_tmp", "write_rows", "target_mask", "reference_mask", "ranks",
                                    "target_age", "reference_age"])
def test_cli_options_refused_with_samples(cli_dir, option):
    r = run_samples(cli_dir, SAMPLES, "E", device=False, more=[f"--{option}", "1"])
    assert r.returncode == 1 and f"--{option} cannot be combined with --mode mut_interval --samples" in r.stderr, r.stderr[-800:]
    assert not list(cli_dir.glob("E_*"))
