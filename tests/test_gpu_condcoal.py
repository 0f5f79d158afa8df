"""`Colate --mode CondCoalRates` on the device (condcoal_kernel.hip): the accumulators against the host twin (1e-12
relative, zeros identical), run-to-run bitwise reproducibility, N = 8192 with a caterpillar tree, and the CLI against the
reference's tables.  Every GPU step runs in a child process under a time limit of its own."""
import os

import numpy as np
import pytest

import condcoal_lib as cl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cl.CASES)
def test_cli_device_matches_reference(case, tmp_path):
    out = str(tmp_path / "out.txt")
    r = cl.run_case(case, out, device=True, timeout=300, extra=())
    assert r.returncode == 0, r.stderr[-2000:]
    worst = cl.compare_tables(out, os.path.join(cl.case_dir(case), "expected.txt"))
    print(f"{case}: largest relative difference of a finite rate {worst:.3e}")
    host = str(tmp_path / "host.txt")
    r = cl.run_case(case, host, device=False, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cl.compare_tables(out, host, rel_tol=1e-6)


def test_cli_reports_the_device(tmp_path):
    out = str(tmp_path / "out.txt")
    env_case = cl.run_case("modern", out, device=True, timeout=300)
    assert env_case.returncode == 0
    os.environ["COLATE_TIMING"] = "1"
    try:
        r = cl.run_case("modern", out, device=True, timeout=300)
    finally:
        del os.environ["COLATE_TIMING"]
    assert "device kernels" in r.stderr, r.stderr[-1000:]


@pytest.mark.parametrize("ancient", [False, True])
def test_device_equals_host_twin_large(ancient, tmp_path):
    # modern: N = 1000, 2000 trees, every haplotype of groups 0 / 1 focal / conditional; ancient: the same trees with
    # fewer focal haplotypes (the host twin walks every member of every sibling subtree there)
    inp = cl.random_input(41 + ancient, 1000, 2000, 4, ancient=ancient, caterpillar_at=7, num_blocks=5,
                          n_focal=12 if ancient else None, n_cond=60 if ancient else None)
    epochs, efocal = cl.default_epochs()
    dnum, dden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=True, timeout=300)
    hnum, hden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=False, timeout=600)
    assert (hnum != 0).any()
    cl.assert_close(dnum, hnum)
    cl.assert_close(dden, hden)
    # the same launch again: the same bits
    dnum2, dden2 = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=True, timeout=300)
    assert np.array_equal(dnum.view(np.uint64), dnum2.view(np.uint64))
    assert np.array_equal(dden.view(np.uint64), dden2.view(np.uint64))


@pytest.mark.parametrize("kind", ["empty_cond", "same_group"])
def test_device_equals_host_twin_groups(kind, tmp_path):
    inp = cl.random_input(77, 300, 200, 3, ancient=(kind == "empty_cond"), num_blocks=2, n_focal=40)
    inp["cond"] = np.zeros(0, dtype=np.int32) if kind == "empty_cond" else inp["focal"]
    epochs, efocal = cl.default_epochs(lineage_bin=3.5)
    dnum, dden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=True, timeout=300)
    hnum, hden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=False, timeout=600)
    cl.assert_close(dnum, hnum)
    cl.assert_close(dden, hden)


def test_n8192_with_caterpillar(tmp_path):
    inp = cl.random_input(8, 8192, 3, 128, caterpillar_at=1, num_blocks=1)
    assert 40 <= inp["focal"].size <= 100 and 40 <= inp["cond"].size <= 100
    epochs, efocal = cl.default_epochs()
    dnum, dden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=True, timeout=300)
    hnum, hden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=False, timeout=600)
    assert (hnum != 0).any()
    cl.assert_close(dnum, hnum)
    cl.assert_close(dden, hden)
