"""The CondCoalRates walk (condcoal_walk.hpp) at its edges, on the host twin, bit for bit: inputs on a dyadic grid
(condcoal_edges_lib.py: every addend and every partial sum is exact in double, so the order of summation cannot hide or
excuse a difference) put node heights and sample ages on epoch and focal-epoch boundaries, tie merges, and leave ancient
samples above coalescences.  The literal model counts what the inputs exercise; every comparison is of the bit patterns."""
import numpy as np
import pytest

import colate_amd
import condcoal_edges_lib as el


def _host(inp, epochs, efocal):
    return colate_amd.condcoal_accumulate(epochs=epochs, epochs_focal=efocal, device=False, **inp)


@pytest.mark.parametrize("case", el.CPU_CASES, ids=el.cpu_case_id)
def test_host_twin_equals_literal_model_bitwise(case):
    inp, epochs, efocal = el.cpu_input(case)
    mnum, mden, _ = el.cpu_model(case)
    num, den = _host(inp, epochs, efocal)
    assert el.same_bits(num, mnum)
    assert el.same_bits(den, mden)
    if case[3] >= 24:
        assert (mnum != 0).any() and (mden != 0).any()


def test_matrix_covers_the_walks_edges():
    """Counted by the literal model on the matrix's inputs, where each event happens."""
    total = el.cpu_coverage()
    print("coverage:", {k: total.get(k, 0) for k in el.COVERAGE})
    missing = [k for k in el.COVERAGE if total.get(k, 0) <= 0]
    assert not missing, missing


def _all_pairs(G):
    fg = [a for a in range(G) for _ in range(G)] + list(range(G))
    cg = [b for _ in range(G) for b in range(G)] + [-1] * G
    return fg, cg


@pytest.mark.parametrize("ancient", [False, True], ids=["modern", "ancient"])
def test_host_pairs_equal_host_singles_bitwise(ancient):
    G = 4
    inp = el.dyadic_input(90 + ancient, 24, 6, G, ancient, efocal=el.EFOCALS[3], caterpillar_at=1, shuffled_at=2, num_blocks=3)
    fg, cg = _all_pairs(G)
    kw = {k: inp[k] for k in ("parents", "branch_lengths", "factors", "blocks", "num_blocks", "group_of_hap", "num_groups",
                              "sample_ages")}
    num, den = colate_amd.condcoal_accumulate_pairs(focal_group=fg, cond_group=cg, epochs=el.EPOCHS, epochs_focal=el.EFOCALS[3],
                                                    device=False, **kw)
    assert (num != 0).any()
    for p, (f, c) in enumerate(zip(fg, cg)):
        focal = np.flatnonzero(inp["group_of_hap"] == f)
        cond = np.flatnonzero(inp["group_of_hap"] == c)
        snum, sden = colate_amd.condcoal_accumulate(focal=focal, cond=cond, epochs=el.EPOCHS, epochs_focal=el.EFOCALS[3],
                                                    device=False, **kw)
        assert el.same_bits(num[p], snum), (f, c)
        assert el.same_bits(den[p], sden), (f, c)


# blocks of the chunking cases: blocks that end inside chunks and chunks that end inside blocks; a block index with no tree
CHUNK_BLOCKS = {
    "six_blocks": (np.repeat(np.arange(6), [4, 1, 9, 2, 15, 10]), 6),
    "gaps": (np.repeat([0, 2, 5], [7, 1, 9]), 7),
}


@pytest.mark.parametrize("layout", sorted(CHUNK_BLOCKS))
@pytest.mark.parametrize("ancient", [False, True], ids=["modern", "ancient"])
def test_host_chunks_equal_unchunked_bitwise(ancient, layout, monkeypatch):
    blocks, nb = CHUNK_BLOCKS[layout]
    inp = el.dyadic_input(95 + ancient, 24, blocks.size, 4, ancient, blocks=blocks, num_blocks=nb, caterpillar_at=3)
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    num, den = _host(inp, el.EPOCHS, el.EFOCALS[2])
    present = np.isin(np.arange(nb), blocks)
    assert (num[present] != 0).any(axis=(1, 2, 3)).all()
    assert not num[~present].any() and not den[~present].any()
    fg, cg = _all_pairs(4)
    kw = {k: v for k, v in inp.items() if k not in ("focal", "cond")}
    pnum, pden = colate_amd.condcoal_accumulate_pairs(focal_group=fg, cond_group=cg, epochs=el.EPOCHS,
                                                      epochs_focal=el.EFOCALS[2], device=False, **kw)
    assert el.same_bits(pnum[1], num) and el.same_bits(pden[1], den)  # pair (0, 1): the single run's focal and cond
    for chunk in ("1", "3"):
        monkeypatch.setenv("COLATE_CONDCOAL_CHUNK_TREES", chunk)
        cnum, cden = _host(inp, el.EPOCHS, el.EFOCALS[2])
        assert el.same_bits(cnum, num) and el.same_bits(cden, den), chunk
        qnum, qden = colate_amd.condcoal_accumulate_pairs(focal_group=fg, cond_group=cg, epochs=el.EPOCHS,
                                                          epochs_focal=el.EFOCALS[2], device=False, **kw)
        assert el.same_bits(qnum, pnum) and el.same_bits(qden, pden), chunk


def test_restated_launch_rules():
    """The restatements that the GPU cases lean on, on layouts worked out by hand."""
    assert el.unit_start([3, 253, 300, 1]) == ([0, 3, 256, 556, 557], [0, 256, 556, 557])
    assert el.unit_start([256, 256]) == ([0, 256, 512], [0, 256, 512])
    assert el.unit_start([100, 100, 100]) == ([0, 100, 200, 300], [0, 200, 300])
    assert el.unit_layout([3, 253, 300]) == (True, True, True)
    assert el.unit_layout([256, 300]) == (False, True, False)
    assert el.unit_layout([100, 100]) == (False, False, True)
    assert el.slab_grid(70, 2 * 2 * 31 * 128) == 66 and el.slab_grid(3, 2 * 2 * 31 * 128) == 3
    assert el.slab_grid(5000, 2 * 2 * 7 * 2) == 1024
    assert el.launch_pieces([0] * 5) == [5]
    assert el.launch_pieces([0, 1, 2, 3, 4, 4]) == [6]       # four closes: one piece
    assert el.launch_pieces([0, 1, 2, 3, 4, 5, 5]) == [5, 2]  # the fifth close starts a piece
