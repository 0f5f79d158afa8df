"""`Colate --mode CondCoalRates --pairs` on the host twin (no GPU): the pairs ABI against the single-pair ABI bit for bit,
every --pairs table byte for byte against its single run, the tables against the reference's (tests/golden/ccpairs_*),
and the errors of the list and the options."""
import json
import os

import numpy as np
import pytest

import ccpairs_lib as pl
import colate_amd
import condcoal_lib as cl


def _all_ordered(G):
    fg = [a for a in range(G) for _ in range(G)]
    cg = [b for _ in range(G) for b in range(G)]
    return fg, cg


# kind: (seed, N, T, G, ancient, caterpillar tree, pairs (focal groups, conditional groups))
ABI_KINDS = {
    "modern": (1, 40, 7, 3, False, None, ([0, 1, 2], [1, 2, 0])),
    "ancient": (2, 36, 5, 3, True, None, ([0, 2, 1], [1, 1, 2])),
    "empty_cond": (3, 30, 5, 3, False, None, ([0, 1, 2, 0], [-1, -1, 0, 1])),
    "empty_cond_ancient": (4, 30, 5, 3, True, None, ([1, 2], [-1, 0])),
    "same_group": (5, 30, 5, 4, False, None, ([0, 1, 3], [0, 1, 3])),
    "caterpillar": (6, 48, 5, 3, False, 2, ([0, 1, 2, 2], [1, 0, 2, -1])),
    "g16_all_pairs": (7, 64, 4, 16, False, 1, _all_ordered(16)),
}


@pytest.mark.parametrize("kind", sorted(ABI_KINDS))
def test_host_pairs_abi_equals_single_abi_bitwise(kind):
    seed, N, T, G, ancient, cat, (fg, cg) = ABI_KINDS[kind]
    inp = cl.random_input(seed, N, T, G, ancient=ancient, caterpillar_at=cat, num_blocks=3)
    gh = inp["group_of_hap"]
    gh[:G] = np.arange(G)  # every group has a haplotype
    assert inp["factors"][-1] == -1.0  # the extra pass of the last tree
    epochs, efocal = cl.default_epochs(lineage_bin=3.5)
    num, den, one = pl.accumulate_pairs_and_singles(inp, fg, cg, epochs, efocal, device=False)
    assert num.shape == (len(fg), 3, 2, epochs.size, G)
    assert (num != 0).any() and (den != 0).any()
    for p, (a, b) in enumerate(one):
        assert np.array_equal(pl.bits(num[p]), pl.bits(a)), (kind, p)
        assert np.array_equal(pl.bits(den[p]), pl.bits(b)), (kind, p)


def test_host_pairs_abi_small_chunks(monkeypatch):
    inp = cl.random_input(9, 30, 9, 3, num_blocks=4)
    epochs, efocal = cl.default_epochs()
    fg, cg = _all_ordered(3)
    ref, rden, _ = pl.accumulate_pairs_and_singles(inp, fg, cg, epochs, efocal, device=False, singles=False)
    monkeypatch.setenv("COLATE_CONDCOAL_CHUNK_TREES", "2")
    num, den, one = pl.accumulate_pairs_and_singles(inp, fg, cg, epochs, efocal, device=False)
    assert np.array_equal(pl.bits(num), pl.bits(ref)) and np.array_equal(pl.bits(den), pl.bits(rden))
    for p, (a, b) in enumerate(one):
        assert np.array_equal(pl.bits(num[p]), pl.bits(a)) and np.array_equal(pl.bits(den[p]), pl.bits(b))


def test_pairs_abi_rejects_bad_groups_and_blocks():
    inp = cl.random_input(3, 12, 3, 2, num_blocks=2)
    inp["group_of_hap"][:2] = [0, 1]
    epochs, efocal = cl.default_epochs()
    kw = {k: inp[k] for k in ("parents", "branch_lengths", "factors", "blocks", "num_blocks", "group_of_hap", "num_groups",
                              "sample_ages")}
    for fg, cg in (([2], [0]), ([-1], [0]), ([0], [2]), ([0], [-2]), ([], [])):
        with pytest.raises(colate_amd.ColateError) as e:
            colate_amd.condcoal_accumulate_pairs(focal_group=fg, cond_group=cg, epochs=epochs, epochs_focal=efocal,
                                                 device=False, **kw)
        assert e.value.code == -1, (fg, cg)
    bad = dict(kw, blocks=np.array([1, 0, 1], dtype=np.int32))
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.condcoal_accumulate_pairs(focal_group=[0], cond_group=[1], epochs=epochs, epochs_focal=efocal, device=False,
                                             **bad)
    assert e.value.code == -1
    # a focal group without haplotypes
    g3 = dict(kw, num_groups=3)
    with pytest.raises(colate_amd.ColateError):
        colate_amd.condcoal_accumulate_pairs(focal_group=[2], cond_group=[0], epochs=epochs, epochs_focal=efocal, device=False,
                                             **g3)


@pytest.mark.parametrize("case", ["modern", "ancient", "chr", "mask", "boot"])
def test_cli_pairs_host_twin_equals_single_runs(case, tmp_path):
    pl.copy_dir(cl.case_dir(case), tmp_path)
    shared = pl.strip_single(json.load(open(os.path.join(cl.case_dir(case), "case.json")))["args"])
    groups = pl.groups_of(tmp_path / "in.poplabels")
    tokens = [f"{a},{b}" for a in groups for b in groups] + [f"{groups[-1]},PZZ", groups[0]]
    for g, p, s in pl.pairs_vs_singles(tmp_path, shared, tokens, device=False):
        assert open(p, "rb").read() == open(s, "rb").read(), g


def test_cli_pairs_host_twin_small_chunks(tmp_path):
    """Chunks of two trees: the same bytes."""
    pl.copy_dir(cl.case_dir("chr"), tmp_path)
    shared = pl.strip_single(json.load(open(os.path.join(cl.case_dir("chr"), "case.json")))["args"])
    res = pl.pairs_vs_singles(tmp_path, shared, ["PA,PB", "PC,PA", "PB,PB"], device=False, COLATE_CONDCOAL_CHUNK_TREES="2")
    for g, p, s in res:
        assert open(p, "rb").read() == open(s, "rb").read(), g


@pytest.mark.parametrize("case", pl.CASES)
def test_cli_pairs_host_twin_matches_reference(case, tmp_path):
    d = pl.case_dir(case)
    pairs = pl.case_pairs(case)
    assert len(pairs) >= 10
    outs = [(g, str(tmp_path / f"o{k}.txt")) for k, (g, _) in enumerate(pairs)]
    pl.write_list(tmp_path / "list.txt", outs)
    r = pl.run(d, pl.case_args(case) + ["--pairs", str(tmp_path / "list.txt")], device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    for (g, exp), (_, out) in zip(pairs, outs):
        cl.compare_tables(out, os.path.join(d, exp))


def test_reference_fixtures_cover_the_issue():
    assert {"modern5", "ancient", "chr_boot"} <= set(pl.CASES)
    groups = pl.groups_of(os.path.join(pl.case_dir("modern5"), "in.poplabels"))
    assert len(groups) >= 5
    toks = {g for g, _ in pl.case_pairs("modern5")}
    assert {f"{a},{b}" for a in groups for b in groups} <= toks


def _base(tmp_path):
    pl.copy_dir(cl.case_dir("modern"), tmp_path)
    return ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels", "--lineage_bin", "4"]


def test_unknown_focal_group_is_an_error_before_any_output(tmp_path):
    base = _base(tmp_path)
    (tmp_path / "list.txt").write_text("PA,PB a.txt\nPB,PC b.txt\nPX,PA x.txt\n")
    r = pl.run(tmp_path, base + ["--pairs", "list.txt"], device=False)
    assert r.returncode != 0
    assert "groups not found" in r.stderr and "line 3" in r.stderr, r.stderr[-1000:]
    for f in ("a.txt", "b.txt", "x.txt"):
        assert not (tmp_path / f).exists()


@pytest.mark.parametrize("extra", [["--groups", "PA,PB"], ["--output", "o.txt"], ["-o", "o.txt"]])
def test_pairs_excludes_groups_and_output(extra, tmp_path):
    base = _base(tmp_path)
    (tmp_path / "list.txt").write_text("PA,PB a.txt\n")
    r = pl.run(tmp_path, base + ["--pairs", "list.txt"] + extra, device=False)
    assert r.returncode != 0 and "--pairs" in r.stderr, r.stderr[-1000:]
    assert not (tmp_path / "a.txt").exists() and not (tmp_path / "o.txt").exists()


@pytest.mark.parametrize("text, line", [
    ("PA,PB a.txt\n\nPB,PC a.txt\n", 3),          # duplicate output
    ("PA,PB a.txt\nPB,PC b.txt extra\n", 2),      # three tokens
    ("PA,PB a.txt\n\n\nPB\n", 4),                  # one token
])
def test_malformed_list_reports_its_line(text, line, tmp_path):
    base = _base(tmp_path)
    (tmp_path / "list.txt").write_text(text)
    r = pl.run(tmp_path, base + ["--pairs", "list.txt"], device=False)
    assert r.returncode != 0 and f"line {line}" in r.stderr, r.stderr[-1000:]
    assert not (tmp_path / "a.txt").exists()


def test_empty_list_is_an_error(tmp_path):
    base = _base(tmp_path)
    (tmp_path / "list.txt").write_text("\n  \n")
    r = pl.run(tmp_path, base + ["--pairs", "list.txt"], device=False)
    assert r.returncode != 0 and "no pairs" in r.stderr, r.stderr[-1000:]
