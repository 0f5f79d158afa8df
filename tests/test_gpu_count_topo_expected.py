"""colate_topo_expected_blocks on the GPU against its host twin in every integer -- on the fixture for every block size and set of
epochs, on rows whose block boundaries lie inside a word, on a word and on a tile's boundary, at one base per block, on counts at the
edges of 16 bits laid across word boundaries --, its qualifying rows against the device's own colate_topo_profile_blocks, the
chunking, and `Colate --mode count_topo --samples --age_profile --expected` on the device path against the host's bytes.  The cases
are those of count_topo_jackknife_lib.py; tests/test_count_topo_expected_cpu.py checks the twin against the contract."""
import os

import numpy as np
import pytest

import colate_amd
import count_topo_expected_lib as xl
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl

pytestmark = pytest.mark.gpu

EPOCHS = jl.epochs_sets()


@pytest.mark.parametrize("E", sorted(EPOCHS))
@pytest.mark.parametrize("nbpb", jl.NBPB)
def test_fixture_device_equals_twin_in_every_integer(nbpb, E):
    case = jl.fixture_case()[0]
    got = xl.expected(case, EPOCHS[E], nbpb, device=True)
    xl.assert_same(got, xl.expected(case, EPOCHS[E], nbpb, device=False))
    assert got[1][..., 2].sum(axis=(1, 2)).min() > 0 and (got[1][..., :2] % xl.ONE).any()


@pytest.mark.parametrize("E", (1, 11, 1024))
def test_block_boundaries_inside_a_word_on_a_word_and_on_the_tile(E):
    """the rows of the jackknife's edge case; E = 1 puts every lane of a word on one LDS address, E = 1024 uses the whole histogram"""
    c = jl.edge_case()
    ep = pl.EPOCHS[E]
    got = xl.expected(c, ep, jl.B, device=True)
    xl.assert_same(got, xl.expected(c, ep, jl.B, device=False))
    blk_off, counts = got
    assert colate_amd.topo_expected_blocks_chunks() == 1
    assert not counts[1].any()
    rows_of = np.bincount(jl.row_blocks(c, jl.B, blk_off), minlength=int(blk_off[-1]))
    assert (counts[0, :, :, 2].sum(axis=1) == rows_of).all()  # every row of every block, in its own block
    sparse = np.bincount(jl.row_blocks(c, jl.B, blk_off)[list(jl.SPARSE_ROWS)], minlength=int(blk_off[-1]))
    assert (counts[2, :, :, 2].sum(axis=1) == sparse).all() and sparse.tolist()[:6] == [1, 2, 1, 1, 1, 1]
    _, profiled, _ = jl.profile_blocks(c, ep, jl.B, device=True)  # the qualifying rows are the device's own profile's
    assert (counts[..., 2] == profiled[..., 2]).all()
    assert counts[0, :, :, 0].sum() > 100 * xl.ONE and counts[0, :, :, 1].sum() > 100 * xl.ONE


def test_one_base_per_block_and_the_regrouping():
    """more than 10 000 blocks, most of them one row or none"""
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    whole_nbpb = 1000 * jl.B
    fine = xl.expected(c, ep, 1, device=True)
    xl.assert_same(fine, xl.expected(c, ep, 1, device=False))
    assert 10_000 < fine[0][-1] <= 65535
    mid, whole = xl.expected(c, ep, jl.B, device=True), xl.expected(c, ep, whole_nbpb, device=True)
    assert (jl.regroup(fine[1], fine[0], 1, mid[0], jl.B) == mid[1]).all()
    assert (jl.regroup(fine[1], fine[0], 1, whole[0], whole_nbpb) == whole[1]).all()


def test_extreme_counts_across_word_boundaries():
    c, combos = xl.extreme_case()
    for nbpb, E in ((400, 1), (400, 11), (1, 1)):
        got = xl.expected(c, pl.EPOCHS[E], nbpb, device=True)
        xl.assert_same(got, xl.expected(c, pl.EPOCHS[E], nbpb, device=False))
    # the last one, one base per block and one epoch: a block is a row, and the device's quotient is Python's
    per_row = got[1][0, (c["rows"]["pos"] - 1).astype(np.int64), 0, :].tolist()
    for (a, b, d, e), x in zip(combos, per_row[40:40 + len(combos)]):
        assert x == [a * e * xl.ONE // ((a + b) * (d + e)), b * d * xl.ONE // ((a + b) * (d + e)), 1], ((a, b, d, e), x)


@pytest.mark.parametrize("E", (1, 1024))
def test_one_triple_alone(E):
    c = jl.edge_case()
    for p in range(3):
        alone = dict(c, triples=c["triples"][p:p + 1])
        got = xl.expected(alone, pl.EPOCHS[E], jl.B, device=True)
        xl.assert_same(got, xl.expected(alone, pl.EPOCHS[E], jl.B, device=False))
        assert got[1].shape == (1, 13, E, 3)


def test_one_triple_per_chunk_gives_the_integers_of_the_default_budget():
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    P = len(c["triples"])
    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        one = xl.expected(c, ep, jl.B, device=True)
        assert colate_amd.topo_expected_blocks_chunks() == 1
        os.environ["COLATE_TOPO_BUDGET"] = "1"
        each = xl.expected(c, ep, jl.B, device=True)
        assert colate_amd.topo_expected_blocks_chunks() == P
        assert colate_amd.topo_expected_blocks_kernel_seconds() > 0
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old
    xl.assert_same(each, one)
    xl.assert_same(one, xl.expected(c, ep, jl.B, device=False))


def test_samples_cli_on_the_device_writes_the_hosts_bytes(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--age_profile", jl.BINS, "--expected", "--jackknife", "--block_bases",
              "5000000"]
    case = jl.fixture_case()[0]
    nb = int(colate_amd.topo_blocks(case["row_off"], case["rows"], 5_000_000)[-1])
    r = tl.run_cli(tmp_path, common + ["-o", "H"], tl.HOST)
    assert r.returncode == 0 and f"14 triples expected in {nb} blocks on the host" in r.stderr, r.stderr[-800:]
    r = tl.run_cli(tmp_path, common + ["-o", "D"])
    assert r.returncode == 0, r.stderr[-800:]
    assert f"5 samples staged, 14 triples expected in {nb} blocks on the device\n" in r.stderr and "on the host" not in r.stderr, r.stderr[-800:]
    for name in ("expected", "expected.jackknife"):
        data = (tmp_path / f"H.{name}.txt").read_bytes()
        assert len(data.splitlines()) == 14 * (23 if name == "expected" else 24)
        assert (tmp_path / f"D.{name}.txt").read_bytes() == data, name
    assert sorted(f.name for f in tmp_path.glob("D[._]*")) == ["D.expected.jackknife.txt", "D.expected.txt"]
