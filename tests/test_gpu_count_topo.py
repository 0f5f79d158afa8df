"""colate_topo_samples on the GPU against its host twin, bit for bit, and `Colate --mode count_topo` on the device path against
the reference's files.  The cases, their edges and the twin's side are in count_topo_lib.py and tests/test_count_topo_cpu.py
(which checks the twin against the numpy model and that the cases are what they say)."""
import os

import numpy as np
import pytest

import colate_amd
import count_topo_expected_lib as xl
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(tl.cases()))
def test_device_equals_twin_in_every_bit(name):
    """sizes: chromosomes of 0, 1, 63, 64, 65 and 200 searched rows in one call.  tiles: one row below, exactly and one row
    above the tile of the draw kernel, so the ranks run on across chromosome and tile boundaries.  Both: a triple without a
    qualifying row and two where every row qualifies; Q in the last bit of one word and in the first bit of another only; a
    cond index that qualifies where the walk index of the same sample does not hit; one sample as the reference of one triple
    and the target of another; uniforms on a quotient, one float above and below it, rounding to 1.0f against p == 1, 0
    against p == 0; a stream exactly as long as the longest triple needs."""
    c = tl.cases()[name]
    want = tl.topo(c, device=False)
    got = tl.topo(c, device=True)
    tl.assert_same(got, want)
    tl.assert_same(got, tl.modelled(name))
    tl.assert_edges(name, got)
    assert colate_amd.topo_samples_chunks() == 1


def test_a_stream_one_uniform_short_is_refused_on_the_device():
    c = tl.cases()["sizes"]
    with pytest.raises(colate_amd.ColateError, match=f"needed: {2 * c['rows'].size}"):
        tl.topo(dict(c, uniforms=c["uniforms"][:-1]), device=True)


def test_chunking_changes_no_bit():
    c = tl.cases()["tiles"]
    want = tl.topo(c, device=False)
    per_triple = 2 * 8 * int(want[0][-1])
    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        os.environ["COLATE_TOPO_BUDGET"] = str(3 * per_triple + 5)  # three triples per chunk: three chunks for eight triples
        got = tl.topo(c, device=True)
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old
    assert colate_amd.topo_samples_chunks() == 3
    tl.assert_same(got, want)


def test_the_four_device_calls_in_one_process_keep_their_own_counters():
    """The four device entry points on the jackknife's edge case (E = 11, one block per jl.B bases), one after another and then in
    the reverse order, at the default budget and at one triple per chunk: every result is its host twin's in every integer, and
    every call's two getters report that call alone -- its chunks and its kernel time -- whatever ran in between.  Last, each call
    in turn at one triple per chunk with the other three at the default budget, so that the four counts differ."""
    c, ep = jl.edge_case(), pl.EPOCHS[11]
    P = len(c["triples"])
    calls = [(lambda device: tl.topo(c, device=device), colate_amd.topo_samples_chunks, colate_amd.topo_samples_kernel_seconds),
             (lambda device: pl.profile(c, ep, device), colate_amd.topo_profile_chunks, colate_amd.topo_profile_kernel_seconds),
             (lambda device: jl.profile_blocks(c, ep, jl.B, device), colate_amd.topo_profile_blocks_chunks,
              colate_amd.topo_profile_blocks_kernel_seconds),
             (lambda device: xl.expected(c, ep, jl.B, device), colate_amd.topo_expected_blocks_chunks,
              colate_amd.topo_expected_blocks_kernel_seconds)]
    twins = [run(False) for run, _, _ in calls]

    def run_on_device(k, budget):
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if budget is not None:
            os.environ["COLATE_TOPO_BUDGET"] = budget
        got = calls[k][0](True)
        assert len(got) == len(twins[k])
        for x, y in zip(got, twins[k]):
            assert x.dtype == y.dtype and np.issubdtype(x.dtype, np.integer) and np.array_equal(x, y), k

    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        for budget, chunks in ((None, 1), ("1", P)):
            for order in (range(4), reversed(range(4))):
                for k in order:
                    run_on_device(k, budget)
                    assert calls[k][1]() == chunks and calls[k][2]() > 0, (k, budget)
                assert [chunks_of() for _, chunks_of, _ in calls] == [chunks] * 4, budget
                assert all(seconds_of() > 0 for _, _, seconds_of in calls), budget
        for chunked in range(4):
            for k in range(4):
                run_on_device(k, "1" if k == chunked else None)
            assert [chunks_of() for _, chunks_of, _ in calls] == [P if k == chunked else 1 for k in range(4)], chunked
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old


def test_samples_cli_on_the_device_writes_the_references_files(tmp_path):
    meta = tl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    r = tl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", meta["seed"], "-o", "S"])
    assert r.returncode == 0, r.stderr[-800:]
    assert "5 samples staged, 14 triples drawn on the device" in r.stderr and "on the host" not in r.stderr, r.stderr[-800:]
    tl.assert_samples_files(tmp_path, meta, "S")


def test_single_triple_through_the_device_path_writes_the_references_file(tmp_path):
    meta = tl.stage(tmp_path)
    p = meta["triples"][5]
    r = tl.run_cli(tmp_path, ["--mut", "P", "-i", p["cond"], "--target_tmp", p["target"], "--reference_tmp", p["reference"], "--chr", "chr.txt",
                              "--seed", meta["seed"], "-o", "mine.txt"], {"COLATE_DEVICE_TOPO": "1"})
    assert r.returncode == 0, r.stderr[-800:]
    assert "3 samples staged, 1 triples drawn on the device" in r.stderr, r.stderr[-800:]
    assert (tmp_path / "mine.txt").read_bytes() == (tmp_path / p["output"]).read_bytes()
