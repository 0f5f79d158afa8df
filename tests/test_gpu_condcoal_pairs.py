"""`Colate --mode CondCoalRates --pairs` on the device (condcoal_pairs_kernel.hip): each pair's accumulators bit for bit
those of the single-pair device path, run-to-run reproducible, within 1e-12 of the host twin, and the CLI's tables byte for
byte those of single device runs and within 1e-4 of the reference's.  Every GPU step runs in a child process under a time
limit of its own."""
import json
import os

import numpy as np
import pytest

import ccpairs_lib as pl
import condcoal_lib as cl

pytestmark = pytest.mark.gpu


def _all_ordered(G):
    return [a for a in range(G) for _ in range(G)], [b for _ in range(G) for b in range(G)]


# kind: (seed, N, T, G, ancient, caterpillar tree, blocks, pairs, chunk trees (COLATE_CONDCOAL_CHUNK_TREES))
KINDS = {
    "modern": (51, 500, 60, 10, False, None, 3, _all_ordered(10), None),
    "ancient": (52, 300, 30, 4, True, None, 2, ([0, 1, 2, 3, 0], [1, 2, 3, 0, 2]), None),
    "empty_cond": (53, 200, 40, 3, False, None, 2, ([0, 1, 2], [-1, -1, 1]), None),
    "same_group": (54, 200, 40, 3, True, None, 2, ([0, 1, 2], [0, 1, 2]), None),
    "g16_all_pairs": (55, 400, 12, 16, False, 3, 3, _all_ordered(16), None),
    "n8192_caterpillar": (56, 8192, 3, 128, False, 1, 1, ([0, 5, 7, 127], [1, 5, -1, 0]), None),
    "small_chunks": (57, 300, 41, 5, False, 2, 6, _all_ordered(5), 3),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_device_pairs_equal_single_device_bitwise(kind, tmp_path):
    seed, N, T, G, ancient, cat, nb, (fg, cg), chunk = KINDS[kind]
    inp = cl.random_input(seed, N, T, G, ancient=ancient, caterpillar_at=cat, num_blocks=nb)
    inp["group_of_hap"][:G] = np.arange(G)
    if kind == "small_chunks":  # blocks change inside chunks and chunks end inside blocks
        inp["blocks"] = np.repeat(np.arange(nb), [4, 1, 9, 2, 15, 10]).astype(np.int32)
    epochs, efocal = cl.default_epochs()
    env = {"COLATE_CONDCOAL_CHUNK_TREES": str(chunk)} if chunk else None
    num, den, snum, sden = pl.in_child(tmp_path, inp, fg, cg, epochs, efocal, device=True, timeout=600, env=env)
    assert (num != 0).any()
    assert np.array_equal(pl.bits(num), pl.bits(snum)), kind
    assert np.array_equal(pl.bits(den), pl.bits(sden)), kind
    if kind in ("modern", "small_chunks"):  # the same launch again: the same bits
        num2, den2, _, _ = pl.in_child(tmp_path, inp, fg, cg, epochs, efocal, device=True, timeout=300, singles=False, env=env)
        assert np.array_equal(pl.bits(num), pl.bits(num2)) and np.array_equal(pl.bits(den), pl.bits(den2))
    if kind != "n8192_caterpillar":  # the host twin: within 1e-12, zeros identical
        hnum, hden, _, _ = pl.in_child(tmp_path, inp, fg, cg, epochs, efocal, device=False, timeout=900, singles=False)
        cl.assert_close(num, hnum)
        cl.assert_close(den, hden)


@pytest.mark.parametrize("case, chunk", [("modern", None), ("ancient", None), ("boot", None), ("chr", "3")])
def test_cli_pairs_device_equals_single_device_runs(case, chunk, tmp_path):
    pl.copy_dir(cl.case_dir(case), tmp_path)
    with open(os.path.join(cl.case_dir(case), "case.json")) as f:
        shared = pl.strip_single(json.load(f)["args"])
    groups = pl.groups_of(tmp_path / "in.poplabels")
    tokens = [f"{a},{b}" for a in groups for b in groups] + [f"{groups[0]},PZZ"]
    extra = {"COLATE_CONDCOAL_CHUNK_TREES": chunk} if chunk else {}
    for g, p, s in pl.pairs_vs_singles(tmp_path, shared, tokens, device=True, timeout=300, **extra):
        assert open(p, "rb").read() == open(s, "rb").read(), g


@pytest.mark.parametrize("case", pl.CASES)
def test_cli_pairs_device_matches_reference(case, tmp_path):
    d = pl.case_dir(case)
    pairs = pl.case_pairs(case)
    outs = [(g, str(tmp_path / f"o{k}.txt")) for k, (g, _) in enumerate(pairs)]
    pl.write_list(tmp_path / "list.txt", outs)
    r = pl.run(d, pl.case_args(case) + ["--pairs", str(tmp_path / "list.txt")], device=True, timeout=300, COLATE_TIMING="1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "device kernels" in r.stderr, r.stderr[-1000:]
    for (g, exp), (_, out) in zip(pairs, outs):
        cl.compare_tables(out, os.path.join(d, exp))
