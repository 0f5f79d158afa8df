"""colate_topo_profile without a device: the host twin against the numpy model of age_epoch over the planes of colate_topo_samples,
its invariants, the rows on the edges of the epochs, the refusals by name, and `Colate --mode count_topo --samples --age_profile`
against the reference's own files aggregated per epoch, on the host twin and on the cursor path."""
import numpy as np
import pytest

import colate_amd
import count_topo_lib as tl
import count_topo_profile_lib as pl

SIZES = sorted(pl.EPOCHS)


# ------------------------------------------------------------------ the host twin against the model
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("name", sorted(pl.cases()))
def test_twin_equals_the_model_and_keeps_the_invariants(name, E):
    c = pl.cases()[name]
    got = pl.profile(c, pl.EPOCHS[E], device=False)
    pl.assert_same(got, pl.modelled(name, E))
    pl.assert_invariants(c, got, pl.twin_planes(name))
    assert got[0].shape == (len(tl.TRIPLES), E, 3)
    if E > 1:  # the rows spread: a profile that falls into one epoch is not what is tested
        assert (got[0][:, :, 2].sum(axis=0) > 0).sum() >= min(E, 8) // 2 + 1


def test_the_cases_are_what_they_say():
    assert np.diff(pl.cases()["long"]["row_off"]).tolist() == [3, 5 * tl.TILE + 3]
    for E in SIZES:
        ep = pl.EPOCHS[E]
        assert ep.size == E and (np.diff(ep) > 0).all() and (ep.astype(np.float32).astype(np.float64) == ep).all()
    counts, _ = pl.modelled("tiles", 1024)
    assert (counts[:, :, 2].sum(axis=0) > 0).sum() > 500  # E = 1024 is not 1024 empty epochs
    one, _ = pl.model(pl.cases()["tiles"], pl.ONE_EPOCH_OF_TWO, pl.twin_planes("tiles"))
    assert not one[:, 1, :].any() and one[tl.ALL_ROWS, 0, 2] == pl.cases()["tiles"]["rows"].size


@pytest.mark.parametrize("E", SIZES)
def test_rows_on_the_edges_of_the_epochs(E):
    """a mid on a boundary lands in the upper epoch, one float below in the lower, one above in the upper; age_begin == age_end
    rows count; below epochs[1] and negative: 0; above the last epoch, +inf and an overflowing sum: E - 1; NaN: 0"""
    c, _ = pl.edge_rows(E)
    pl.assert_edge_rows(E, pl.profile(c, pl.EPOCHS[E], device=False))


def test_all_rows_in_one_epoch():
    c = pl.cases()["tiles"]
    counts, draws = pl.profile(c, pl.ONE_EPOCH_OF_TWO, device=False)
    pl.assert_same((counts, draws), pl.model(c, pl.ONE_EPOCH_OF_TWO, pl.twin_planes("tiles")))
    assert (counts[:, 0, 2] == draws).all() and not counts[:, 1, :].any()


# ------------------------------------------------------------------ refusals
def test_refusals_of_the_call_name_their_argument():
    c = pl.cases()["sizes"]

    def refused(what, epochs, **change):
        with pytest.raises(colate_amd.ColateError, match=what):
            pl.profile(dict(c, **change), epochs, device=False)

    refused("E = 0 epochs", np.zeros(0))
    refused("E = 1025 epochs", np.arange(1025.0))
    refused(r"epochs\[3\] = 2 does not lie above epochs\[2\] = 2", np.array([0.0, 1.0, 2.0, 2.0, 3.0]))
    refused(r"epochs\[1\] = 0 does not lie above epochs\[0\] = 0", np.array([0.0, 0.0, 3.0]))
    refused(r"epochs\[2\] = 1 does not lie above epochs\[1\] = 5", np.array([0.0, 5.0, 1.0]))
    refused(r"epochs\[2\] is not finite", np.array([0.0, 1.0, np.inf]))
    refused(r"epochs\[0\] is not finite", np.array([np.nan, 1.0]))
    refused(f"needed: {2 * c['rows'].size}", pl.EPOCHS[11], uniforms=c["uniforms"][:-1])
    tr = c["triples"].copy()
    tr[3]["target"] = 7
    refused("triple 3: sample id out of range", pl.EPOCHS[11], triples=tr)  # (what colate_topo_samples refuses, through the same checks)
    lib = colate_amd.api.lib
    a = [np.ascontiguousarray(c["row_off"]), np.ascontiguousarray(c["rows"]), np.ascontiguousarray(c["idx"]), np.ascontiguousarray(c["cond_idx"]),
         np.ascontiguousarray(c["triples"]), np.ascontiguousarray(c["uniforms"]), pl.EPOCHS[11].copy()]
    counts, draws = np.full((len(tl.TRIPLES), 11, 3), -7, dtype=np.int64), np.full(len(tl.TRIPLES), -7, dtype=np.int64)
    p = [x.ctypes.data for x in a]

    def call(counts_p, draws_p, epochs_p=p[6]):
        return lib.colate_topo_profile_host(a[0].size - 1, p[0], p[1], 7, p[2], p[3], len(tl.TRIPLES), p[4], a[5].size, p[5], 11, epochs_p, counts_p, draws_p)

    for args in ((None, draws.ctypes.data), (counts.ctypes.data, None), (counts.ctypes.data, draws.ctypes.data, None)):
        assert call(*args) == -1 and "NULL pointer" in lib.colate_last_error().decode()
    assert (counts == -7).all() and (draws == -7).all()  # nothing is written after a refusal
    assert call(counts.ctypes.data, draws.ctypes.data) == 0 and (counts >= 0).all()
    with pytest.raises(ValueError, match="cond_idx must be"):
        colate_amd.topo_profile(c["row_off"], c["rows"], c["idx"], c["cond_idx"][:3], c["triples"], c["uniforms"], pl.EPOCHS[2], device=False)


# ------------------------------------------------------------------ the command line on the reference's files
COMMON = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt"]


def staged(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    return meta


def test_profile_of_the_references_files_on_the_host_twin_and_the_cursor_path(tmp_path):
    meta = staged(tmp_path)
    epochs, _ = colate_amd.epochs_from_bins(pl.BINS)
    E = epochs.size
    assert E == 11
    want = pl.reference_profile(tmp_path, meta, epochs)
    # the reference's lines populate the epochs with both signs: a profile collapsed into one bin cannot pass
    assert ((want[:, :, 0].sum(axis=0) > 0) & (want[:, :, 1].sum(axis=0) > 0)).sum() >= 8
    args = COMMON + ["--seed", meta["seed"], "--age_profile", pl.BINS]
    runs = {"H": (tl.HOST, [], "5 samples staged, 14 triples profiled on the host"), "K": (tl.CURSORS, [], "through the record cursors"),
            "HO": (tl.HOST, ["--profile_only"], "5 samples staged, 14 triples profiled on the host"),
            "KO": (tl.CURSORS, ["--profile_only"], "through the record cursors"), "N": (tl.HOST, None, "14 triples drawn on the host")}
    for out, (env, more, said) in runs.items():
        r = tl.run_cli(tmp_path, (args if more is not None else COMMON + ["--seed", meta["seed"]]) + ["-o", out] + (more or []), env)
        assert r.returncode == 0 and said in r.stderr, r.stderr[-800:]
        assert ("profiled on the" in r.stderr) == (more is not None and env is tl.HOST)
        assert ("drawn on the host\n" in r.stderr) == (more == [] and env is tl.HOST or more is None), r.stderr[-800:]
    printed, counts = pl.read_profile(tmp_path / "H.profile.txt", meta, E)
    assert (counts[:, :, :2] == want).all(), np.argwhere(counts[:, :, :2] != want)[:8]
    assert printed == ["%g" % x for x in epochs]  # in generations, as a .coal prints them
    assert (counts[:, :, 0] + counts[:, :, 1] <= counts[:, :, 2]).all()
    totals = (tmp_path / "H.triples.txt").read_text().splitlines()
    for p, line in enumerate(totals):
        x = line.split(" ")
        assert [int(v) for v in x[3:]] == [counts[p, :, 0].sum(), counts[p, :, 1].sum(), counts[p, :, 2].sum()]
    profile, triples = (tmp_path / "H.profile.txt").read_bytes(), (tmp_path / "H.triples.txt").read_bytes()
    for out in ("K", "HO", "KO"):  # the cursor path, and --profile_only on both: the same bytes
        assert (tmp_path / f"{out}.profile.txt").read_bytes() == profile and (tmp_path / f"{out}.triples.txt").read_bytes() == triples, out
    assert triples == (tmp_path / "N.triples.txt").read_bytes() and not (tmp_path / "N.profile.txt").exists()
    tl.assert_samples_files(tmp_path, meta, "H")
    for t in meta["triples"]:  # the per-triple files: those of a run without the option; none with --profile_only
        name = "_".join(t["names"]) + ".txt"
        assert (tmp_path / f"H_{name}").read_bytes() == (tmp_path / f"N_{name}").read_bytes() == (tmp_path / f"K_{name}").read_bytes()
    for out in ("HO", "KO"):
        assert sorted(f.name for f in tmp_path.glob(out + "*")) == [out + ".profile.txt", out + ".triples.txt"]


def test_years_per_gen_moves_the_epochs(tmp_path):
    meta = staged(tmp_path)
    r = tl.run_cli(tmp_path, COMMON + ["--seed", meta["seed"], "--age_profile", pl.BINS, "--years_per_gen", "25", "--profile_only", "-o", "Y"], tl.HOST)
    assert r.returncode == 0, r.stderr[-800:]
    epochs, _ = colate_amd.epochs_from_bins(pl.BINS, 0.0, 25.0)
    printed, counts = pl.read_profile(tmp_path / "Y.profile.txt", meta, epochs.size)
    assert printed == ["%g" % x for x in epochs] and (counts[:, :, :2] == pl.reference_profile(tmp_path, meta, epochs)).all()


def test_the_three_new_errors_come_before_any_file(tmp_path):
    meta = staged(tmp_path)

    def run(args, env=tl.HOST):
        r = tl.run_cli(tmp_path, args + ["-o", "X"], env)
        assert r.returncode == 1 and not list(tmp_path.glob("X*")), (r.returncode, r.stderr[-500:])
        return r.stderr

    assert "epochs format is wrong. Specify x,y,stepsize." in run(COMMON + ["--age_profile", "3,7"])
    assert "epochs format is wrong. Specify x,y,stepsize." in run(COMMON + ["--age_profile", "a,b,c"])
    assert "--profile_only needs --age_profile" in run(COMMON + ["--profile_only"])
    t = meta["triples"][0]
    single = ["--mut", "P", "-i", t["cond"], "--target_tmp", t["target"], "--reference_tmp", t["reference"], "--chr", "chr.txt"]
    assert "--age_profile needs --mode count_topo --samples" in run(single + ["--age_profile", pl.BINS], None)
    assert "--profile_only needs --mode count_topo --samples" in run(single + ["--profile_only"], None)
    import subprocess
    r = subprocess.run([tl.il.CLI, "--mode", "compare_tmp", "--age_profile", pl.BINS] + COMMON + ["-o", "X"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=60)  # every other mode refuses the two options instead of ignoring them
    assert r.returncode == 1 and "--age_profile is an option of --mode count_topo --samples" in r.stderr and not list(tmp_path.glob("X*"))
