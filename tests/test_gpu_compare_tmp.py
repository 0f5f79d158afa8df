"""colate_compare_samples on the GPU against its host twin, int for int, and `Colate --mode compare_tmp` on the device path
against the reference's files.  The cases, their edges and the twin's side are in compare_tmp_lib.py and
tests/test_compare_tmp_cpu.py (which checks the twin against the numpy model and that the cases are what they say)."""
import os

import pytest

import colate_amd
import compare_tmp_lib as cl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(cl.cases()))
def test_device_equals_twin_in_every_int(name):
    """sizes: chromosomes of 1, 63, 64, 65, 0, 256 and 257 searched rows in one call, window = 7 with three and more window
    boundaries in a word, empty windows inside and behind the rows, positions on first + 7 k and first + 7 k + 1, first_pos
    below the first row, rows at equal positions, prev_bp = -2, records without counts, the first row of a chromosome below
    the last position of the one before.  many_windows: thousands of windows per workgroup.  wide_window: hundreds of words
    per window."""
    c = cl.cases()[name]
    want = cl.compare(c, device=False)
    got = cl.compare(c, device=True)
    cl.assert_same(got, want)
    cl.assert_same(got, cl.modelled(name))
    cl.assert_symmetric(c, got)
    assert colate_amd.compare_samples_chunks() == 1


def test_chunking_changes_no_int():
    c = cl.cases()["many_windows"]
    want = cl.compare(c, device=False)
    per_pair = 2 * 4 * int(want[0][-1])
    old = os.environ.pop("COLATE_COMPARE_BUDGET", None)
    try:
        os.environ["COLATE_COMPARE_BUDGET"] = str(2 * per_pair + 5)  # two pairs per chunk: three chunks for six pairs
        got = cl.compare(c, device=True)
    finally:
        os.environ.pop("COLATE_COMPARE_BUDGET", None)
        if old is not None:
            os.environ["COLATE_COMPARE_BUDGET"] = old
    assert colate_amd.compare_samples_chunks() == 3
    cl.assert_same(got, want)


def test_samples_cli_on_the_device_writes_the_references_files(tmp_path):
    meta = cl.stage(tmp_path)
    (tmp_path / "samples.txt").write_text("\n".join(meta["samples"]) + "\n")
    r = cl.run_cli(tmp_path, ["--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "-o", "S"])
    assert r.returncode == 0, r.stderr[-800:]
    assert "4 samples staged, 7 pairs compared on the device" in r.stderr and "on the host" not in r.stderr, r.stderr[-800:]
    cl.assert_samples_files(tmp_path, meta, "S")


def test_single_pair_through_the_device_path_writes_the_references_file(tmp_path):
    meta = cl.stage(tmp_path)
    p = meta["pairs"][3]
    r = cl.run_cli(tmp_path, ["--mut", "P", "--target_tmp", p["target"], "--reference_tmp", p["reference"], "--chr", "chr.txt", "-o", "mine.txt"],
                   {"COLATE_DEVICE_COMPARE": "1"})
    assert r.returncode == 0, r.stderr[-800:]
    assert "2 samples staged, 1 pairs compared on the device" in r.stderr, r.stderr[-800:]
    assert (tmp_path / "mine.txt").read_bytes() == (tmp_path / p["output"]).read_bytes()
