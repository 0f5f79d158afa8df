"""`CoalRate --mode local_ancestry` on the device (coalrate_kernel.hip): the CLI against the reference's .coal for every
committed fixture, and the raw sums against the host twin bit for bit over small and large N, one and many groups, modern
and ancient samples, chunk and block boundaries, calls that share a workgroup, prefix counts that do not fit the LDS, and
per-block sums that outgrow their device buffers.
Every GPU step runs in a child process under a time limit of its own; a test stops at the first child that fails."""
import os

import numpy as np
import pytest

import coalrate_lib as cl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cl.CASES)
def test_cli_device_matches_reference(name, tmp_path):
    r = cl.run_case(name, str(tmp_path / "out"), device=True, timeout=300, extra_env={"COLATE_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "device kernels" in r.stderr, r.stderr[-1000:]
    total, differ = cl.compare_coal(str(tmp_path / "out.coal"), os.path.join(cl.case_dir(name), "expected.coal"))
    print(f"{name}: {total} rate tokens, {differ} not identical")
    # and the host twin's file, byte for byte
    r = cl.run_case(name, str(tmp_path / "host"), device=False, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "out.coal") as a, open(tmp_path / "host.coal") as b:
        assert a.read() == b.read()


# N, G, T, S, blocks, ancient, chunk cap (None: the default chunk)
SHAPES = [
    (8, 1, 40, 2, 3, False, 7),
    (8, 2, 5000, 3, 4, True, None),     # T / 1024 >= 2: several calls share a workgroup
    (300, 2, 300, 4, 5, False, 64),
    (300, 26, 120, 3, 4, True, 50),
    (2000, 2, 40, 2, 3, True, 16),
    (2000, 26, 24, 2, 3, False, 10),
    (4000, 26, 12, 2, 3, True, 5),      # 26 x 4001 prefix counts do not fit the LDS: the device-memory path
    (8, 1, 36, 2, 9, False, 4),         # nine blocks in chunks of four: the per-block sums on the device grow four times
]


@pytest.mark.parametrize("N,G,T,S,nb,ancient,cap", SHAPES)
def test_device_equals_host_twin_bit_for_bit(N, G, T, S, nb, ancient, cap, tmp_path):
    if (N, G) == (4000, 26):
        assert 2 * (G * (N + 1) + N) > 160 * 1024
    rng = np.random.default_rng(1000 * N + 10 * G + ancient)
    epochs = cl.bins_epochs(2.0, 6.0, 0.25)
    inp = cl.random_input(rng, N, T, G, S, nb, ancient, epochs) + (nb, G)
    if nb == 9:
        inp = inp[:3] + (cl.GROW_BLOCKS,) + inp[4:]
        assert len(set(inp[3].tolist())) == nb and (inp[2] != 0).all()
        reallocations, copying = cl.sum_reallocations(inp[3], cap)
        assert reallocations >= 3 and copying >= 2      # the sums move to larger buffers with earlier blocks in them
    if cap:
        assert T > cap and len(set(inp[3][:cap].tolist())) + len(set(inp[3].tolist())) > 2  # chunks and blocks are crossed
    dnum, dden, shape = cl.accumulate_in_child(tmp_path, inp, epochs, device=True, timeout=300, chunk_trees=cap, with_shape=True)
    # what the device call did (coalrate_launch_shape): chunks launched, lanes per call, shared workgroups, where the prefix counts lay
    assert shape["launches"] == -(-T // (cap or T)) and shape["lanes_per_call"] == {1: 1, 2: 4, 26: 256}[G], shape
    assert shape["lds"] == ((N, G) != (4000, 26)), shape
    if T == 5000:
        assert shape["cpw_min"] == shape["cpw_max"] >= 2, shape     # several calls share a workgroup
    else:
        assert shape["cpw_min"] == shape["cpw_max"] == 1, shape
    hnum, hden = cl.accumulate_in_child(tmp_path, inp, epochs, device=False, timeout=600, chunk_trees=cap)
    assert (hnum != 0).any() and (hden != 0).any()
    assert np.array_equal(dnum.view(np.uint64), hnum.view(np.uint64))
    assert np.array_equal(dden.view(np.uint64), hden.view(np.uint64))
