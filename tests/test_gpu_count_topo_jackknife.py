"""colate_topo_profile_blocks on the GPU against its host twin in every integer -- on the fixture for every block size and set of
epochs, and on rows whose block boundaries lie inside a word, on a word and on the draw tile's boundary --, its sums against
colate_topo_profile on the device, the chunking, and `Colate --mode count_topo --samples --age_profile --jackknife` on the device
path against the host's bytes.  The cases and the model's side are in count_topo_jackknife_lib.py and
tests/test_count_topo_jackknife_cpu.py (which checks the twin against the reference's own lines)."""
import os

import numpy as np
import pytest

import colate_amd
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl

pytestmark = pytest.mark.gpu

EPOCHS = jl.epochs_sets()


def assert_same(got, want):
    for name, x, y in zip(("blk_off", "counts", "draws"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, x.shape, y.shape, np.argwhere(x != y)[:8])


@pytest.mark.parametrize("E", sorted(EPOCHS))
@pytest.mark.parametrize("nbpb", jl.NBPB)
def test_fixture_device_equals_twin_in_every_integer(nbpb, E):
    """30 000 000 bases: four blocks a chromosome at most; 5 000 000: about twenty; 100 000: most blocks hold one row at most and many
    none.  E = 1 (every add of a block on three addresses), the 23 epochs of 3,7,0.2, and 1024 (the whole histogram of every block)."""
    case = jl.fixture_case()[0]
    got = jl.profile_blocks(case, EPOCHS[E], nbpb, device=True)
    assert_same(got, jl.profile_blocks(case, EPOCHS[E], nbpb, device=False))
    assert (got[1][..., 2].sum(axis=(1, 2)) == got[2]).all() and got[2].min() > 0


@pytest.mark.parametrize("E", (1, 11, 1024))
def test_block_boundaries_inside_a_word_on_a_word_and_on_the_tile(E):
    """2 TILE + 64 + 3 rows: boundaries between rows 37 | 38, 63 | 64 (pos = 2 B next to 2 B + 1), TILE - 2 | TILE - 1 | TILE |
    TILE + 1, two blocks without a row, a last block of the last row alone, three rows at one position; a chromosome without rows
    and one of one row; a triple whose every row qualifies, one without a qualifying row, one with a few"""
    c = jl.edge_case()
    ep = pl.EPOCHS[E]
    want = jl.profile_blocks(c, ep, jl.B, device=False)
    got = jl.profile_blocks(c, ep, jl.B, device=True)
    assert_same(got, want)
    blk_off, counts, draws = got
    assert colate_amd.topo_profile_blocks_chunks() == 1
    assert draws.tolist() == [jl.N0 + 1, 0, len(jl.SPARSE_ROWS)] and not counts[1].any()
    rows_of = np.bincount(jl.row_blocks(c, jl.B, blk_off), minlength=int(blk_off[-1]))
    assert (counts[0, :, :, 2].sum(axis=1) == rows_of).all()  # every row of every block drew, in its own block
    sparse = np.bincount(jl.row_blocks(c, jl.B, blk_off)[list(jl.SPARSE_ROWS)], minlength=int(blk_off[-1]))
    assert (counts[2, :, :, 2].sum(axis=1) == sparse).all() and sparse.tolist()[:6] == [1, 2, 1, 1, 1, 1]
    whole, whole_draws = pl.profile(c, ep, device=True)  # the sums over the blocks are the device's own profile
    assert (counts.sum(axis=1) == whole).all() and (draws == whole_draws).all()
    assert (counts[0, :, :, 0].sum() > 100) and (counts[0, :, :, 1].sum() > 100)


def test_the_draws_of_the_rows_do_not_depend_on_the_blocks():
    """one base per block, B bases, and one block per chromosome: the finer counts regrouped are the coarser ones"""
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    whole_nbpb = 1000 * jl.B
    fine = jl.profile_blocks(c, ep, 1, device=True)
    mid = jl.profile_blocks(c, ep, jl.B, device=True)
    whole = jl.profile_blocks(c, ep, whole_nbpb, device=True)
    assert_same(fine, jl.profile_blocks(c, ep, 1, device=False))
    assert 10_000 < fine[0][-1] <= 65535 and np.diff(whole[0]).tolist() == [1, 1, 1]
    assert (jl.regroup(fine[1], fine[0], 1, mid[0], jl.B) == mid[1]).all()
    assert (jl.regroup(mid[1], mid[0], jl.B, whole[0], whole_nbpb) == jl.regroup(fine[1], fine[0], 1, whole[0], whole_nbpb)).all()
    assert (jl.regroup(fine[1], fine[0], 1, whole[0], whole_nbpb) == whole[1]).all()
    assert (fine[2] == mid[2]).all() and (mid[2] == whole[2]).all()
    # at one base per block a block's qualifying rows are the rows at one position
    assert (fine[1][0, :, :, 2].sum(axis=1) == np.bincount(jl.row_blocks(c, 1, fine[0]), minlength=int(fine[0][-1]))).all()


def test_one_triple_per_chunk_gives_the_integers_of_the_default_budget():
    c = jl.edge_case()
    ep = pl.EPOCHS[11]
    P = len(c["triples"])
    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        one = jl.profile_blocks(c, ep, jl.B, device=True)
        assert colate_amd.topo_profile_blocks_chunks() == 1
        os.environ["COLATE_TOPO_BUDGET"] = "1"
        each = jl.profile_blocks(c, ep, jl.B, device=True)
        assert colate_amd.topo_profile_blocks_chunks() == P
        assert colate_amd.topo_profile_blocks_kernel_seconds() > 0
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old
    assert_same(each, one)
    assert_same(one, jl.profile_blocks(c, ep, jl.B, device=False))


@pytest.mark.parametrize("E", (1, 1024))
def test_one_triple_alone(E):
    c = jl.edge_case()
    for p in range(3):
        alone = dict(c, triples=c["triples"][p:p + 1])
        got = jl.profile_blocks(alone, pl.EPOCHS[E], jl.B, device=True)
        assert_same(got, jl.profile_blocks(alone, pl.EPOCHS[E], jl.B, device=False))
        assert got[1].shape == (1, 13, E, 3)


def test_refusals_on_the_device():
    c = jl.edge_case()
    with pytest.raises(colate_amd.ColateError, match=f"needed: {2 * (jl.N0 + 1)}"):
        jl.profile_blocks(dict(c, uniforms=c["uniforms"][:-1]), pl.EPOCHS[11], jl.B, device=True)
    with pytest.raises(colate_amd.ColateError, match=r"epochs\[2\] = 1 does not lie above epochs\[1\] = 1"):
        jl.profile_blocks(c, [0.0, 1.0, 1.0], jl.B, device=True)
    with pytest.raises(colate_amd.ColateError, match="num_bases_per_block = 0: at least 1"):
        jl.profile_blocks(c, pl.EPOCHS[11], 0, device=True)


def test_samples_cli_on_the_device_writes_the_hosts_bytes(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    common = ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", meta["seed"], "--age_profile", jl.BINS, "--jackknife",
              "--block_bases", "5000000"]
    case = jl.fixture_case()[0]
    nb = int(colate_amd.topo_blocks(case["row_off"], case["rows"], 5_000_000)[-1])
    r = tl.run_cli(tmp_path, common + ["-o", "H"], tl.HOST)
    assert r.returncode == 0 and f"14 triples profiled in {nb} blocks on the host" in r.stderr, r.stderr[-800:]
    r = tl.run_cli(tmp_path, common + ["-o", "D"])
    assert r.returncode == 0, r.stderr[-800:]
    assert "5 samples staged, 14 triples drawn on the device" in r.stderr
    assert f"5 samples staged, 14 triples profiled in {nb} blocks on the device\n" in r.stderr and "on the host" not in r.stderr, r.stderr[-800:]
    r = tl.run_cli(tmp_path, common + ["--profile_only", "-o", "O"])
    assert r.returncode == 0, r.stderr[-800:]
    assert f"5 samples staged, 14 triples profiled in {nb} blocks on the device\n" in r.stderr and "drawn on the" not in r.stderr, r.stderr[-800:]
    want = {name: (tmp_path / f"H.{name}.txt").read_bytes() for name in ("jackknife", "profile", "triples")}
    assert len(want["jackknife"].splitlines()) == 14 * 24
    for out in ("D", "O"):
        for name, data in want.items():
            assert (tmp_path / f"{out}.{name}.txt").read_bytes() == data, (out, name)
    tl.assert_samples_files(tmp_path, meta, "D")
    assert sorted(f.name for f in tmp_path.glob("O*")) == ["O.jackknife.txt", "O.profile.txt", "O.triples.txt"]
