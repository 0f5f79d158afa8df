"""colate_topo_profile on the GPU against its host twin in every integer, and `Colate --mode count_topo --samples --age_profile` on
the device path against the host's bytes.  The cases, the epochs and the model's side are in count_topo_profile_lib.py and
tests/test_count_topo_profile_cpu.py (which checks the twin against the numpy model and the reference's files)."""
import os

import pytest

import colate_amd
import count_topo_lib as tl
import count_topo_profile_lib as pl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("E", sorted(pl.EPOCHS))
@pytest.mark.parametrize("name", sorted(pl.cases()))
def test_device_equals_twin_in_every_integer(name, E):
    """sizes: chromosomes of 0, 1, 63, 64, 65 and 200 searched rows in one call.  tiles: TILE - 1, TILE and TILE + 1 rows.  long:
    5 TILE + 3 rows behind a chromosome of 3: every wave owns a tile, one owns two, the last tile is partial.  All with the
    triples of count_topo_lib: no qualifying row, every row qualifying, Q in a last and a first bit of a word only, samples
    shared between triples in other roles.  E = 1 (every add of a word on one address), 2, 11 and 1024 (the whole histogram)."""
    c = pl.cases()[name]
    want = pl.profile(c, pl.EPOCHS[E], device=False)
    got = pl.profile(c, pl.EPOCHS[E], device=True)
    pl.assert_same(got, want)
    pl.assert_same(got, pl.modelled(name, E))
    pl.assert_invariants(c, got, pl.twin_planes(name))
    assert colate_amd.topo_profile_chunks() == 1


def test_all_rows_of_every_chromosome_in_one_epoch():
    """the 64 lanes of a word whose every row qualifies add to the same three addresses"""
    c = pl.cases()["tiles"]
    got = pl.profile(c, pl.ONE_EPOCH_OF_TWO, device=True)
    pl.assert_same(got, pl.profile(c, pl.ONE_EPOCH_OF_TWO, device=False))
    assert (got[0][:, 0, 2] == got[1]).all() and not got[0][:, 1, :].any() and got[1][tl.ALL_ROWS] == c["rows"].size


@pytest.mark.parametrize("E", sorted(pl.EPOCHS))
def test_rows_on_the_edges_of_the_epochs(E):
    """mids on, one float below and one float above a boundary, age_begin == age_end, negative, infinite, overflowing and NaN
    ages, for three samples in permuted roles: the device's float addition and comparison are the host's"""
    c, _ = pl.edge_rows(E)
    got = pl.profile(c, pl.EPOCHS[E], device=True)
    pl.assert_same(got, pl.profile(c, pl.EPOCHS[E], device=False))
    pl.assert_edge_rows(E, got)


def test_a_stream_one_uniform_short_and_bad_epochs_are_refused_on_the_device():
    c = pl.cases()["sizes"]
    with pytest.raises(colate_amd.ColateError, match=f"needed: {2 * c['rows'].size}"):
        pl.profile(dict(c, uniforms=c["uniforms"][:-1]), pl.EPOCHS[11], device=True)
    with pytest.raises(colate_amd.ColateError, match=r"epochs\[2\] = 1 does not lie above epochs\[1\] = 1"):
        pl.profile(c, [0.0, 1.0, 1.0], device=True)


def test_chunking_changes_no_integer():
    c = pl.cases()["tiles"]
    E = 11
    want = pl.profile(c, pl.EPOCHS[E], device=False)
    C, P = c["row_off"].size - 1, len(c["triples"])
    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        one = pl.profile(c, pl.EPOCHS[E], device=True)
        assert colate_amd.topo_profile_chunks() == 1
        os.environ["COLATE_TOPO_BUDGET"] = str(12 * E * C)  # the partials of one triple: a chunk per triple
        each = pl.profile(c, pl.EPOCHS[E], device=True)
        assert colate_amd.topo_profile_chunks() == P
        os.environ["COLATE_TOPO_BUDGET"] = str(3 * 12 * E * C + 5)  # three triples per chunk, the last chunk short
        three = pl.profile(c, pl.EPOCHS[E], device=True)
        assert colate_amd.topo_profile_chunks() == (P + 2) // 3
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old
    for got in (one, each, three):
        pl.assert_same(got, want)


def test_samples_cli_on_the_device_writes_the_hosts_bytes(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", meta["seed"], "--age_profile", pl.BINS]
    r = tl.run_cli(tmp_path, common + ["-o", "H"], tl.HOST)
    assert r.returncode == 0 and "14 triples profiled on the host" in r.stderr, r.stderr[-800:]
    r = tl.run_cli(tmp_path, common + ["-o", "D"])
    assert r.returncode == 0, r.stderr[-800:]
    assert "5 samples staged, 14 triples drawn on the device" in r.stderr and "5 samples staged, 14 triples profiled on the device" in r.stderr
    assert "on the host" not in r.stderr, r.stderr[-800:]
    r = tl.run_cli(tmp_path, common + ["--profile_only", "-o", "O"])
    assert r.returncode == 0, r.stderr[-800:]
    assert "5 samples staged, 14 triples profiled on the device" in r.stderr and "drawn on the" not in r.stderr, r.stderr[-800:]
    profile, triples = (tmp_path / "H.profile.txt").read_bytes(), (tmp_path / "H.triples.txt").read_bytes()
    assert len(profile) > 14 * 11 * 10
    for out in ("D", "O"):
        assert (tmp_path / f"{out}.profile.txt").read_bytes() == profile and (tmp_path / f"{out}.triples.txt").read_bytes() == triples, out
    tl.assert_samples_files(tmp_path, meta, "D")
    assert sorted(f.name for f in tmp_path.glob("O*")) == ["O.profile.txt", "O.triples.txt"]
