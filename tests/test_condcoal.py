"""`Colate --mode CondCoalRates` on the host twin (no GPU): readers, epochs, the factorised walk against the literal
restatement of the reference (condcoal_model.py), and the CLI against the reference's tables (tests/golden/condcoal_*,
written by golden/make_golden_condcoal.py)."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import colate_amd
import condcoal_lib as cl
import condcoal_model as cm


@pytest.mark.parametrize("case", cl.CASES)
def test_cli_host_twin_matches_reference(case, tmp_path):
    out = str(tmp_path / "out.txt")
    r = cl.run_case(case, out, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    worst = cl.compare_tables(out, os.path.join(cl.case_dir(case), "expected.txt"))
    print(f"{case}: largest relative difference of a finite rate {worst:.3e}")


def test_fixture_set_is_complete():
    for c in ("modern", "ancient", "empty_cond", "same_group", "default_lineage", "bins", "chr", "mask", "boot", "large"):
        assert c in cl.CASES


def _copy_case(case, dst):
    src = cl.case_dir(case)
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), dst)


def _run(cwd, args, device=False):
    env = dict(os.environ, COLATE_DEVICE_CONDCOAL="0")
    return subprocess.run([cl.CLI, "--mode", "CondCoalRates"] + args, cwd=cwd, capture_output=True, text=True, env=env,
                          timeout=300)


def test_plain_and_gz_anc_read_alike(tmp_path):
    _copy_case("modern", tmp_path)
    base = ["--input", "in", "--poplabels", "in.poplabels", "--groups", "PB,PC", "--lineage_bin", "4"]
    assert _run(tmp_path, base + ["-o", "gz.txt"]).returncode == 0
    for ext in ("anc", "mut"):
        with gzip.open(tmp_path / f"in.{ext}.gz", "rb") as f, open(tmp_path / f"in.{ext}", "wb") as g:
            g.write(f.read())
        os.remove(tmp_path / f"in.{ext}.gz")
    assert _run(tmp_path, base + ["-o", "plain.txt"]).returncode == 0
    assert (tmp_path / "gz.txt").read_text() == (tmp_path / "plain.txt").read_text()


def test_ages_kept_only_when_all_present(tmp_path):
    """NUM_HAPLOTYPES N a_1 .. a_k with k != N: the ages are dropped (the modern path)."""
    _copy_case("ancient", tmp_path)
    with gzip.open(tmp_path / "in.anc.gz", "rt") as f:
        lines = f.read().splitlines(True)
    head = lines[0].split()
    base = ["--input", "in", "--poplabels", "in.poplabels", "--groups", "PA,PB", "--lineage_bin", "4"]
    assert _run(tmp_path, base + ["-o", "anc.txt"]).returncode == 0
    with open(tmp_path / "in.anc", "w") as f:
        f.write(" ".join(head[:-1]) + "\n" + "".join(lines[1:]))  # one age short
    os.remove(tmp_path / "in.anc.gz")
    assert _run(tmp_path, base + ["-o", "short.txt"]).returncode == 0
    with open(tmp_path / "in.anc", "w") as f:
        f.write(" ".join(head[:2]) + "\n" + "".join(lines[1:]))  # no ages
    assert _run(tmp_path, base + ["-o", "none.txt"]).returncode == 0
    assert (tmp_path / "short.txt").read_text() == (tmp_path / "none.txt").read_text()
    assert (tmp_path / "anc.txt").read_text() != (tmp_path / "none.txt").read_text()


def test_groups_sorted_and_epochs_as_reference():
    """The group column lists the poplabels' second column sorted; epoch.start is the reference's float grid."""
    exp = open(os.path.join(cl.case_dir("modern"), "expected.txt")).read().splitlines()[1:]
    groups = [l.split()[3] for l in exp[:4]]
    assert groups == sorted(groups) == ["PA", "PB", "PC", "PD"]
    starts = []
    for l in exp[::4]:
        s = l.split()[2]
        if l.split()[1] == "0":
            starts.append(s)
    epochs, _ = cl.default_epochs()
    assert starts == ["%g" % float(e) for e in epochs]
    bins = open(os.path.join(cl.case_dir("bins"), "expected.txt")).read().splitlines()[1:]
    assert len({l.split()[2] for l in bins}) == 7  # 0, 10^3 .. 10^4.5 (4), 10^5, max(1e8, 10 x last)


def test_default_lineage_bin_prints_inf():
    exp = open(os.path.join(cl.case_dir("default_lineage"), "expected.txt")).read().splitlines()[1:]
    assert {l.split()[1] for l in exp} == {"0", "inf"}


@pytest.mark.parametrize("kind", ["modern", "ancient", "empty_cond", "empty_cond_ancient", "same_group", "caterpillar"])
def test_host_twin_equals_literal_model(kind):
    N, T, G = 24, 6, 4
    inp = cl.random_input(5 + len(kind), N, T, G, ancient="ancient" in kind,
                          caterpillar_at=2 if kind == "caterpillar" else None, num_blocks=2)
    if kind.startswith("empty_cond"):
        inp["cond"] = np.zeros(0, dtype=np.int32)
    if kind == "same_group":
        inp["cond"] = inp["focal"]
    # one tree with its internal labels out of coalescence order (root kept at 2N-2)
    rng = np.random.default_rng(1)
    p = inp["parents"][1].copy()
    perm = np.arange(2 * N - 1)
    perm[N:2 * N - 2] = rng.permutation(np.arange(N, 2 * N - 2))
    newp = np.full_like(p, -1)
    newb = np.zeros(2 * N - 1)
    for v in range(2 * N - 1):
        newb[perm[v]] = inp["branch_lengths"][1][v]
        if p[v] >= 0:
            newp[perm[v]] = perm[p[v]]
    inp["parents"][1], inp["branch_lengths"][1] = newp, newb
    assert any(newp[v] >= 0 and newp[v] < v for v in range(N, 2 * N - 1))
    epochs, efocal = cl.default_epochs(lineage_bin=3.5)
    num, den = colate_amd.condcoal_accumulate(epochs=epochs, epochs_focal=efocal, device=False, **inp)
    mnum = np.zeros_like(num)
    mden = np.zeros_like(den)
    for t in range(T):
        a, b = cm.tree_accumulators(inp["parents"][t], inp["branch_lengths"][t], inp["factors"][t], inp["group_of_hap"], G,
                                    inp["focal"], inp["cond"], epochs, efocal, inp["sample_ages"])
        mnum[inp["blocks"][t]] += a
        mden[inp["blocks"][t]] += b
    assert (mnum != 0).any() and (mden != 0).any()
    cl.assert_close(num, mnum)
    cl.assert_close(den, mden)


def test_rejects_map_and_dist(tmp_path):
    _copy_case("modern", tmp_path)
    base = ["--input", "in", "--poplabels", "in.poplabels", "--groups", "PB,PC", "-o", "x.txt"]
    r = _run(tmp_path, base + ["--map", "genmap.txt"])
    assert r.returncode != 0 and "--map" in r.stderr
    r = _run(tmp_path, base + ["--dist", "in.dist"])
    assert r.returncode != 0 and "dist" in r.stderr
    assert not (tmp_path / "x.txt").exists()


def test_bad_trees_and_sizes_are_errors():
    inp = cl.random_input(3, 8, 2, 2, num_blocks=1)
    epochs, efocal = cl.default_epochs()
    bad = dict(inp)
    bad["parents"] = inp["parents"].copy()
    bad["parents"][0][-1] = 9  # no root at 2N-2
    with pytest.raises(colate_amd.ColateError):
        colate_amd.condcoal_accumulate(epochs=epochs, epochs_focal=efocal, device=False, **bad)
    big = 16385
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.condcoal_accumulate(np.full((1, 2 * big - 1), -1), np.zeros((1, 2 * big - 1)), [1.0], [0], 1,
                                       np.zeros(big), 1, [0], [1], epochs, efocal, device=False)
    assert e.value.code == -4  # COLATE_ELIMIT
