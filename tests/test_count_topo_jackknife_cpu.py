"""colate_topo_blocks, colate_topo_profile_blocks and colate_topo_jackknife without a device, and `Colate --mode count_topo --samples
--age_profile --jackknife` on the host twin and on the cursor path: the counts per (block, epoch) against the reference's own lines
binned here, their sums against colate_topo_profile, the blocks against a three-line restatement, the statistic against the plain
Python of topo_jackknife_model.py in every bit and against its textbook form, the files of the command line, and the refusals."""
import math

import numpy as np
import pytest

import colate_amd
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl
import topo_jackknife_model as model

EPOCHS = jl.epochs_sets()


def same_stats(got, want, negated=False):
    """every double in every bit (a NaN equals a NaN).  negated: `want` is the negative of a result, and a zero keeps its sign --
    (double)0 / n is +0 whichever way plus and minus lie"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    alike = np.isnan(got) & np.isnan(want)
    if negated:
        alike |= (got == 0) & (want == 0)
    assert ((got.view(np.uint64) == want.view(np.uint64)) | alike).all(), (got, want)


# ------------------------------------------------------------------ the fixture: blocks x epochs against the reference's lines
@pytest.mark.parametrize("E", sorted(EPOCHS))
@pytest.mark.parametrize("nbpb", jl.NBPB)
def test_fixture_counts_sum_to_the_profile_and_equal_the_references_lines_per_block(nbpb, E):
    case = jl.fixture_case()[0]
    epochs = EPOCHS[E]
    blk_off, counts, draws = jl.profile_blocks(case, epochs, nbpb, device=False)
    assert (blk_off == jl.blocks_model(case["row_off"], case["rows"]["pos"], nbpb)).all()
    assert counts.shape == (14, int(blk_off[-1]), E, 3) and counts.dtype == np.int64
    whole, whole_draws = pl.profile(case, epochs, device=False)
    assert (counts.sum(axis=1) == whole).all() and (draws == whole_draws).all()
    want = jl.reference_blocks(epochs, nbpb, blk_off)
    jl.assert_equals_reference(counts, want)
    if nbpb == 100_000:  # most blocks hold one row at most and many hold none
        per_block = np.bincount(jl.row_blocks(case, nbpb, blk_off), minlength=int(blk_off[-1]))
        assert (per_block == 0).sum() > 100 and (per_block <= 1).mean() > 0.5
    if E == 23:  # the lines spread over blocks and epochs with both signs: counts collapsed into one cell cannot pass
        assert len({k[2] for k in want}) >= 8 and len({k[1] for k in want}) >= min(int(blk_off[-1]), 8) and {k[3] for k in want} == {0, 1}


def test_the_fixture_is_the_one_the_issue_names():
    case, meta, chroms, _ = jl.fixture_case()
    n = np.diff(case["row_off"])
    # (three .mut files of 900 to 1105 rows, of which the mode searches these)
    assert len(chroms) == 3 and n.min() >= 800 and n.max() <= 1105 and len(meta["triples"]) == 14 and int(meta["seed"]) == 5
    assert 90_000_000 < case["rows"]["pos"].max() <= 95_000_000
    totals = {}
    for p, _, sign in jl.reference_lines():
        totals[p, sign] = totals.get((p, sign), 0) + 1
    for p, t in enumerate(meta["triples"]):  # every line of the reference found its row
        assert (totals[p, 1], totals[p, -1]) == (t["plus"], t["minus"])


# ------------------------------------------------------------------ the blocks
def test_blocks_against_the_restatement():
    """a chromosome without rows owns one block; a gap leaves empty blocks; pos = k nbpb is the last base of block k - 1 and
    k nbpb + 1 the first of block k; equal positions share a block; pos <= 0 lies in block 0"""
    nbpb = 100
    chroms = [[1, 50, 100, 101, 101, 101, 200, 201], [], [7, 1000], [100], [101], [0, 0, 3], [99, 100, 100, 101, 950]]
    row_off = np.concatenate([[0], np.cumsum([len(c) for c in chroms])]).astype(np.int64)
    rows = np.zeros(int(row_off[-1]), dtype=colate_amd.WALK_ROW)
    rows["pos"] = [p for c in chroms for p in c]
    got = colate_amd.topo_blocks(row_off, rows, nbpb)
    assert got.dtype == np.int32 and (got == jl.blocks_model(row_off, rows["pos"], nbpb)).all()
    assert np.diff(got).tolist() == [3, 1, 10, 1, 2, 1, 10]
    for nbpb in (1, 7, 100, 1000, 10 ** 9):
        assert (colate_amd.topo_blocks(row_off, rows, nbpb) == jl.blocks_model(row_off, rows["pos"], nbpb)).all()
    case = jl.edge_case()
    off = colate_amd.topo_blocks(case["row_off"], case["rows"], jl.B)
    assert np.diff(off).tolist() == [11, 1, 1]
    per_block = np.bincount(jl.row_blocks(case, jl.B, off), minlength=13)
    assert per_block[7] == 0 and per_block[8] == 0 and per_block[3] == 1 and per_block[4] == 1 and per_block[10] == 1 and per_block[11] == 0
    first = np.concatenate([[0], np.cumsum(per_block)])[:11]
    assert sorted(set(first.tolist())) == sorted(set(jl.FIRST_ROWS) | {7000})  # (the two empty blocks start where block 9 does)


def test_blocks_refusals():
    row_off = np.array([0, 2], dtype=np.int64)
    rows = np.zeros(2, dtype=colate_amd.WALK_ROW)
    rows["pos"] = [5, 70000]
    with pytest.raises(colate_amd.ColateError, match="num_bases_per_block = 0: at least 1"):
        colate_amd.topo_blocks(row_off, rows, 0)
    with pytest.raises(colate_amd.ColateError, match=r"needed: 70000"):
        colate_amd.topo_blocks(row_off, rows, 1)
    assert colate_amd.topo_blocks(row_off, rows, 2)[-1] == 35000
    rows["pos"] = [5, 2 ** 31 - 10 ** 6]
    with pytest.raises(colate_amd.ColateError, match=r"position 2146483648 at or above 2\^31 - num_bases_per_block"):
        colate_amd.topo_blocks(row_off, rows, 10 ** 6)
    assert colate_amd.topo_blocks(row_off, rows, 10 ** 6 - 1)[-1] == (2 ** 31 - 10 ** 6 - 1) // (10 ** 6 - 1) + 1  # one base fewer: taken


def test_profile_blocks_refusals_by_name_and_nothing_written():
    c = jl.edge_case()
    ep = pl.EPOCHS[11]

    def refused(what, epochs=ep, nbpb=jl.B, **change):
        with pytest.raises(colate_amd.ColateError, match=what):
            jl.profile_blocks(dict(c, **change), epochs, nbpb, device=False)

    refused("E = 0 epochs", np.zeros(0))
    refused("E = 1025 epochs", np.arange(1025.0))
    refused(r"epochs\[2\] = 1 does not lie above epochs\[1\] = 5", np.array([0.0, 5.0, 1.0]))
    refused(r"epochs\[1\] is not finite", np.array([0.0, np.inf]))
    refused(f"needed: {2 * (jl.N0 + 1)}", uniforms=c["uniforms"][:-1])
    tr = c["triples"].copy()
    tr[1]["target"] = 4
    refused("triple 1: sample id out of range", triples=tr)
    refused("num_bases_per_block = 0: at least 1", nbpb=0)
    lib = colate_amd.api.lib
    a = [np.ascontiguousarray(c[k]) for k in ("row_off", "rows", "idx", "cond_idx", "triples", "uniforms")] + [ep.copy()]
    p = [x.ctypes.data for x in a]
    nb = int(colate_amd.topo_blocks(c["row_off"], c["rows"], jl.B)[-1])
    counts, draws = np.full((3, nb + 1, 11, 3), -7, dtype=np.int64), np.full(3, -7, dtype=np.int64)

    def call(nb_given, counts_p=counts.ctypes.data, draws_p=draws.ctypes.data, nbpb=jl.B):
        return lib.colate_topo_profile_blocks_host(3, p[0], p[1], 4, p[2], p[3], 3, p[4], a[5].size, p[5], 11, p[6], nbpb, nb_given, counts_p, draws_p)

    assert call(nb + 1) == -1 and f"nb = {nb + 1} is not the {nb} blocks of these rows" in lib.colate_last_error().decode()
    assert call(nb - 1) == -1 and f"nb = {nb - 1} is not the {nb} blocks" in lib.colate_last_error().decode()
    assert call(nb, None) == -1 and "NULL pointer" in lib.colate_last_error().decode()
    assert call(nb, counts.ctypes.data, None) == -1 and "NULL pointer" in lib.colate_last_error().decode()
    assert (counts == -7).all() and (draws == -7).all()
    assert call(nb) == 0 and (counts.reshape(-1)[:3 * nb * 33] >= 0).all() and (draws == [jl.N0 + 1, 0, len(jl.SPARSE_ROWS)]).all()
    # the most a call takes, E = 1024 with 65535 blocks, lies under the 1 GB of one triple's partials: it is not refused
    rows = np.zeros(1, dtype=colate_amd.WALK_ROW)
    rows["pos"] = 65535
    idx = np.zeros((1, 1), dtype=colate_amd.WALK_IDX)
    blk_off, big, _ = colate_amd.topo_profile_blocks([0, 1], rows, idx, idx, [(0, 0, 0)], np.zeros(2), np.arange(1024.0), 1, device=False)
    assert blk_off[-1] == 65535 and big.shape == (1, 65535, 1024, 3) and not big.any()


# ------------------------------------------------------------------ the statistic
def random_counts(rng, nb, E, empty=0.2, top=60):
    c = rng.integers(0, top, (nb, E, 3)).astype(np.int64)
    c[rng.uniform(size=(nb, E)) < empty, :2] = 0
    c[..., 2] += c[..., 0] + c[..., 1]
    return c


def test_jackknife_equals_the_plain_python_model_in_every_bit():
    case = jl.fixture_case()[0]
    for nbpb in jl.NBPB[:2]:
        _, counts, _ = jl.profile_blocks(case, EPOCHS[23], nbpb, device=False)
        for p in range(counts.shape[0]):
            stats, used = colate_amd.topo_jackknife(counts[p])
            want, want_used = model.jackknife(counts[p].tolist())
            same_stats(stats, want)
            assert used.tolist() == want_used
        assert np.isfinite(colate_amd.topo_jackknife(counts[0])[0][-1]).all()  # `all` of a fixture triple has D, D_jack, se and Z
    rng = np.random.default_rng(17)
    for nb, E, top in ((1, 1, 9), (2, 3, 9), (7, 5, 60), (40, 4, 10 ** 6), (12, 2, 2 ** 40), (300, 2, 4)):
        for _ in range(4):
            c = random_counts(rng, nb, E, top=top)
            stats, used = colate_amd.topo_jackknife(c)
            want, want_used = model.jackknife(c.tolist())
            same_stats(stats, want)
            assert used.tolist() == want_used and stats.shape == (E + 1, 4) and used.dtype == np.int32


def test_jackknife_with_equal_block_sizes_is_the_textbook_delete_one():
    rng = np.random.default_rng(23)
    for g in (2, 5, 16, 60):
        n_j = int(rng.integers(20, 400))
        a = rng.integers(0, n_j + 1, g)
        c = np.zeros((g + 2, 1, 3), dtype=np.int64)  # two blocks without a line among them: not used
        at = np.sort(rng.choice(g + 2, g, replace=False))
        c[at, 0, 0], c[at, 0, 1] = a, n_j - a
        stats, used = colate_amd.topo_jackknife(c)
        assert used.tolist() == [g, g]
        A, M = int(a.sum()), int((n_j - a).sum())
        theta = [(A - int(x) - (M - (n_j - int(x)))) / (A + M - n_j) for x in a]
        mean = math.fsum(theta) / g
        var = (g - 1) / g * math.fsum((t - mean) ** 2 for t in theta)
        D = (A - M) / (A + M)
        D_jack = g * D - (g - 1) * mean
        for cell in (0, 1):
            assert stats[cell, 0] == D
            assert abs(stats[cell, 1] - D_jack) <= 1e-9 * max(abs(D_jack), 1e-300) or abs(stats[cell, 1] - D_jack) < 1e-15
            assert abs(stats[cell, 2] - math.sqrt(var)) <= 1e-9 * math.sqrt(var)


def test_jackknife_of_identical_blocks():
    for g in (2, 3, 7, 16):
        for a, b in ((5, 3), (0, 9), (11, 11), (1000003, 17)):
            c = np.zeros((g, 2, 3), dtype=np.int64)
            c[:, :, 0], c[:, :, 1] = a, b
            stats, used = colate_amd.topo_jackknife(c)
            assert used.tolist() == [g] * 3
            for D, D_jack, se, Z in stats:
                assert D == (a - b) / (a + b) and abs(D_jack - D) <= 1e-12 and abs(se) <= 1e-12
                assert math.isnan(Z) if se == 0 else math.isfinite(Z)
    c = np.zeros((4, 1, 3), dtype=np.int64)
    c[:, 0, 0], c[:, 0, 1] = 6, 2  # (h - 1 = 3, theta = D = 0.5: every operation exact, se is 0 and Z not available)
    stats, _ = colate_amd.topo_jackknife(c)
    assert stats[0, 0] == 0.5 and stats[0, 1] == 0.5 and stats[0, 2] == 0.0 and math.isnan(stats[0, 3])


def test_swapping_plus_and_minus_negates_d_and_z_in_every_bit():
    rng = np.random.default_rng(29)
    for nb, E in ((2, 1), (9, 4), (50, 3)):
        c = random_counts(rng, nb, E)
        s = c.copy()
        s[..., 0], s[..., 1] = c[..., 1], c[..., 0]
        (x, ux), (y, uy) = colate_amd.topo_jackknife(c), colate_amd.topo_jackknife(s)
        assert ux.tolist() == uy.tolist()
        same_stats(y[:, [0, 1, 3]], -x[:, [0, 1, 3]], negated=True)
        same_stats(y[:, 2], x[:, 2])
        assert nb < 9 or np.isfinite(x[-1]).all()


def test_jackknife_nan_rules_and_refusals():
    c = np.zeros((5, 3, 3), dtype=np.int64)
    c[2, 1, :] = 4, 1, 9     # epoch 1: one used block
    c[:, 2, 2] = 7            # epoch 2: qualifying rows but no line
    stats, used = colate_amd.topo_jackknife(c)
    assert used.tolist() == [0, 1, 0, 1]
    assert np.isnan(stats[0]).all() and np.isnan(stats[2]).all()
    for cell in (1, 3):
        assert stats[cell, 0] == 0.6 and np.isnan(stats[cell, 1:]).all()
    with pytest.raises(ValueError, match=r"counts must be \[nb\]\[E\]\[3\]"):
        colate_amd.topo_jackknife(np.zeros((3, 3), dtype=np.int64))
    c[0, 0, 1] = -1
    with pytest.raises(colate_amd.ColateError, match=r"counts\[1\] = -1 is negative"):
        colate_amd.topo_jackknife(c)
    lib = colate_amd.api.lib
    out, u = np.zeros(8), np.zeros(2, dtype=np.int32)
    ok = np.ones((1, 1, 3), dtype=np.int64)
    assert lib.colate_topo_jackknife(0, 1, ok.ctypes.data, out.ctypes.data, u.ctypes.data) == -1 and "nb=0" in lib.colate_last_error().decode()
    assert lib.colate_topo_jackknife(1, 1, ok.ctypes.data, None, u.ctypes.data) == -1 and "NULL pointer" in lib.colate_last_error().decode()


# ------------------------------------------------------------------ the command line
COMMON = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt"]


def staged(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    return meta


def modelled_file(nbpb):
    """PREFIX.jackknife.txt as the Python model prints it from the library's counts on the fixture read here"""
    case, meta, _, _ = jl.fixture_case()
    _, counts, _ = jl.profile_blocks(case, EPOCHS[23], nbpb, device=False)
    printed = ["%g" % x for x in colate_amd.epochs_from_bins(jl.BINS)[0]]
    out = []
    for p, t in enumerate(meta["triples"]):
        out += model.lines(" ".join(t["names"]), printed, counts[p].tolist())
    return "".join(line + "\n" for line in out)


def test_cli_files_with_jackknife_are_those_without_and_the_three_forms_agree(tmp_path):
    meta = staged(tmp_path)
    args = COMMON + ["--seed", meta["seed"], "--age_profile", jl.BINS]
    jk = ["--jackknife", "--block_bases", "5000000"]
    runs = {"N": (tl.HOST, []), "H": (tl.HOST, jk), "K": (tl.CURSORS, jk), "NO": (tl.HOST, ["--profile_only"]),
            "HO": (tl.HOST, jk + ["--profile_only"]), "KO": (tl.CURSORS, jk + ["--profile_only"]), "HD": (tl.HOST, ["--jackknife"])}
    for out, (env, more) in runs.items():
        r = tl.run_cli(tmp_path, args + ["-o", out] + more, env)
        assert r.returncode == 0, (out, r.stderr[-800:])
        assert ("triples profiled in " in r.stderr) == ("--jackknife" in more and env is tl.HOST), (out, r.stderr[-800:])
        if env is tl.HOST and "--jackknife" in more:
            case = jl.fixture_case()[0]
            nb = int(colate_amd.topo_blocks(case["row_off"], case["rows"], 30_000_000 if out == "HD" else 5_000_000)[-1])
            assert f"5 samples staged, 14 triples profiled in {nb} blocks on the host\n" in r.stderr
            assert "profiled on the" not in r.stderr
    files = lambda out: sorted(f.name[len(out):] for f in tmp_path.glob(out + "[._]*"))  # noqa: E731
    for with_jk, without in (("H", "N"), ("K", "N"), ("HO", "NO"), ("KO", "NO"), ("HD", "N")):
        assert files(with_jk) == sorted(files(without) + [".jackknife.txt"])
        for name in files(without):  # profile.txt, triples.txt and every per-triple file: byte for byte
            assert (tmp_path / (with_jk + name)).read_bytes() == (tmp_path / (without + name)).read_bytes(), (with_jk, name)
    assert files("NO") == [".profile.txt", ".triples.txt"] and len(files("N")) == 2 + 14
    want = modelled_file(5_000_000)
    assert len(want.splitlines()) == 14 * 24 and " all " in want and "NA" in want
    for out in ("H", "K", "HO", "KO"):
        assert (tmp_path / f"{out}.jackknife.txt").read_text() == want, out
    assert (tmp_path / "HD.jackknife.txt").read_text() == modelled_file(30_000_000) != want  # the default: 30 000 000 bases
    zs = [line.split(" ")[10] for line in want.splitlines() if line.split(" ")[3] == "all"]
    assert len(zs) == 14 and all(z != "NA" and math.isfinite(float(z)) for z in zs)  # every triple's `all` line carries a Z


def test_cli_errors_come_before_any_file(tmp_path):
    meta = staged(tmp_path)

    def run(args, env=tl.HOST, code=1):
        r = tl.run_cli(tmp_path, args + ["-o", "X"], env)
        assert r.returncode == code and not list(tmp_path.glob("X*")), (r.returncode, r.stderr[-500:], list(tmp_path.glob("X*")))
        return r.stderr

    prof = COMMON + ["--age_profile", jl.BINS]
    assert "Error: --jackknife needs --age_profile x,y,stepsize." in run(COMMON + ["--jackknife"])
    assert "Error: --block_bases needs --jackknife." in run(prof + ["--block_bases", "1000"])
    for bad in ("0", "-5", "1.5", "3e7", "abc", "10x", "", "99999999999"):
        assert f"Error: --block_bases takes an integer of at least 1 (given: {bad})." in run(prof + ["--jackknife", "--block_bases", bad])
    t = meta["triples"][0]
    single = ["--mut", "P", "-i", t["cond"], "--target_tmp", t["target"], "--reference_tmp", t["reference"], "--chr", "chr.txt"]
    assert "--jackknife needs --mode count_topo --samples" in run(single + ["--jackknife"], None)
    assert "--block_bases needs --mode count_topo --samples" in run(single + ["--block_bases", "5"], None)
    # the library's refusals by name: more than 65535 blocks, on the host twin and on the cursor path
    for env in (tl.HOST, tl.CURSORS):
        err = run(prof + ["--jackknife", "--block_bases", "1000"], env)
        assert "blocks of 1000 bases, 65535 are possible (needed: " in err, err[-500:]
    import subprocess
    r = subprocess.run([tl.il.CLI, "--mode", "compare_tmp", "--jackknife"] + COMMON + ["-o", "X"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=60)  # every other mode refuses the two options instead of ignoring them
    assert r.returncode == 1 and "--jackknife is an option of --mode count_topo --samples" in r.stderr and not list(tmp_path.glob("X*"))
