"""`CoalRate --mode tree` on the device (coalrate_tree_kernel.hip): the CLI against the reference's .coal for every
committed fixture, and the raw sums against the host twin bit for bit from three keys to the path beyond the LDS, with ties,
node times on epoch boundaries, ancient samples, calls that share a workgroup, chunk and block boundaries, and per-block
sums that outgrow their device buffers.  Every GPU step runs in a child process under a time limit of its own; a test stops
at the first child that fails."""
import os

import numpy as np
import pytest

import coalrate_lib as cl
import coalrate_tree_lib as tl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tl.EXPECTED_CASES)
def test_cli_device_matches_reference(name, tmp_path):
    r = tl.run_case(name, str(tmp_path / "out"), device=True, timeout=300, extra_env={"COLATE_TIMING": "1", "COLATE_DEVICE_COALRATE": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "device kernels" in r.stderr, r.stderr[-1000:]
    total, differ = cl.compare_coal(str(tmp_path / "out.coal"), os.path.join(tl.case_dir(name), "expected.coal"))
    print(f"{name}: {total} rate tokens, {differ} not identical")
    # and the host twin's file, byte for byte
    r = tl.run_case(name, str(tmp_path / "host"), device=False, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "out.coal") as a, open(tmp_path / "host.coal") as b:
        assert a.read() == b.read()


# N, T, blocks, ancient, quantum (None: continuous heights), chunk cap (None: the default chunk)
SHAPES = [
    (2, 40, 3, False, None, 7),        # three keys
    (8, 9000, 4, True, None, 4499),    # chunks above the wave slots: calls share a workgroup, the last one partly filled
    (300, 60, 4, True, 64.0, 25),      # padding to 1024 keys; ties and boundary-equal times
    (2000, 40, 3, True, None, 16),     # ancient samples; chunk cap 16
    (8192, 4, 2, False, None, None),   # the last N that sorts in LDS
    (12000, 6, 2, True, None, 4),      # the path beyond the LDS
    (8, 36, 9, False, None, 4),        # nine blocks in chunks of four: the per-block sums on the device grow four times
]


@pytest.mark.parametrize("N,T,nb,ancient,quantum,cap", SHAPES)
def test_device_equals_host_twin_bit_for_bit(N, T, nb, ancient, quantum, cap, tmp_path):
    P = tl.padded_keys(N)
    if N == 2:
        assert 2 * N - 1 == 3
    if N == 300:
        assert P == 1024 and 2 * N - 1 < P
    if N == 8192:
        assert P == tl.LDS_KEYS and tl.padded_keys(N + 1) > tl.LDS_KEYS
    if N == 12000:
        assert P > tl.LDS_KEYS
    rng = np.random.default_rng(77 * N + ancient)
    epochs = tl.TIE_EPOCHS if quantum else cl.bins_epochs(2.0, 6.0, 0.25)
    inp = tl.random_input(rng, N, T, nb, ancient, epochs, quantum, Ne=300.0 if quantum is None and N >= 2000 else 2000.0)
    if nb == 9:
        inp = inp[:3] + (cl.GROW_BLOCKS,) + inp[4:]
        assert len(set(inp[3].tolist())) == nb and (inp[2] != 0).all()
        reallocations, copying = cl.sum_reallocations(inp[3], cap)
        assert reallocations >= 3 and copying >= 2      # the sums move to larger buffers with earlier blocks in them
    if cap:
        assert T > cap and tl.chunk_straddles_blocks(inp[3], cap)   # chunks are crossed, and block boundaries inside them
    dnum, dden, shape = tl.accumulate_in_child(tmp_path, inp, nb, epochs, device=True, timeout=300, chunk_trees=cap, with_shape=True)
    # what the device call did (coalrate_tree_launch_shape), not what a restated rule predicts
    assert shape["launches"] == -(-T // (cap or T)) and shape["lanes_per_call"] == min(256, max(4, P // 2)), shape
    assert shape["lds"] == (P <= tl.LDS_KEYS), shape
    if N == 8 and T == 9000:
        assert shape["cpw_max"] >= 2, shape                       # more calls in a chunk than wave slots: workgroups are shared
        assert cap % shape["cpw_max"] != 0 and T > 2 * cap, shape   # the last workgroup of a chunk is partly filled
        assert shape["cpw_min"] == 1, shape                       # and the last chunk, of two calls, is not packed
    else:
        assert shape["cpw_min"] == shape["cpw_max"] == 1, shape
    hnum, hden = tl.accumulate_in_child(tmp_path, inp, nb, epochs, device=False, timeout=600, chunk_trees=cap)
    assert (hnum != 0).any() and (hden != 0).any()
    assert np.array_equal(dnum.view(np.uint64), hnum.view(np.uint64))
    assert np.array_equal(dden.view(np.uint64), hden.view(np.uint64))
