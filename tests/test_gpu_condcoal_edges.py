"""The two CondCoalRates kernels (condcoal_kernel.hip, condcoal_pairs_kernel.hip) at the edges of their launch logic, bit
for bit: the prefix scan's lane chunks (N = 2, 3, 255 .. 513), a second and third batch of focal haplotypes, more trees than
workgroups, a grid capped by the slab limit, chunks of one and three trees with blocks across them and block indices without
a tree, pairs packed into units of exactly and of more than 256 items, and chunks launched in pieces.  All inputs are on
condcoal_edges_lib's dyadic grid, where every sum is exact, so the device, the host twin and (N <= 40) the literal model
must give the same bits.  Every GPU step runs in a child process under a time limit of its own."""
import numpy as np
import pytest

import ccpairs_lib as pl
import colate_amd
import condcoal_edges_lib as el
import condcoal_lib as cl

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("ancient", [False, True], ids=["modern", "ancient"])
CHILD_S = 120  # time limit of a device child


def _check_single(tmp_path, inp, epochs, efocal, env=None, model=False):
    """The single kernel against the host twin (unchunked, in this process: no GPU step) and the literal model."""
    el.assert_exact(inp, epochs, efocal)
    dnum, dden = cl.accumulate_in_child(tmp_path, inp, epochs, efocal, device=True, timeout=CHILD_S, env=env)
    hnum, hden = colate_amd.condcoal_accumulate(epochs=epochs, epochs_focal=efocal, device=False, **inp)
    assert el.same_bits(dnum, hnum)
    assert el.same_bits(dden, hden)
    if model:
        mnum, mden = el.model_accumulate(inp, epochs, efocal)
        assert el.same_bits(dnum, mnum)
        assert el.same_bits(dden, mden)
    return hnum, hden


@MODES
@pytest.mark.parametrize("N, G", [(2, 1), (3, 2)])
def test_s1_smallest_trees(N, G, ancient, tmp_path, monkeypatch):
    """Lanes >= N idle in the prefix scan; N = 2, G = 1: the empty conditional group."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    inp = el.dyadic_input(100 + N, N, 5, G, ancient, efocal=el.EFOCALS[3], shuffled_at=2)
    if G == 1:
        inp = el.with_cond(inp, "empty")
    hnum, _ = _check_single(tmp_path, inp, el.EPOCHS, el.EFOCALS[3], model=True)
    assert (hnum != 0).any()


@MODES
@pytest.mark.parametrize("N", [255, 256, 257, 513])
def test_s2_prefix_lane_chunks(N, ancient, tmp_path, monkeypatch):
    """ceil(N / 256) changes between these N, and trailing lanes get empty ranges."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    inp = el.dyadic_input(200 + N, N, 4, 3, ancient, caterpillar_at=1)
    hnum, _ = _check_single(tmp_path, inp, el.EPOCHS, el.EFOCALS[2])
    assert (hnum != 0).any()


@MODES
@pytest.mark.parametrize("F, kind", [(255, "plain"), (256, "plain"), (257, "plain"), (513, "plain"), (257, "same"), (257, "empty")])
def test_s3_focal_batches(F, kind, ancient, tmp_path, monkeypatch):
    """A second and a third batch of focal haplotypes, a last batch of fewer than 256 rows, the read-back of the tree's
    sums between batches; `same`: every focal haplotype is a conditional too."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    inp = el.dyadic_input(300 + F, 600, 3, 2, ancient, efocal=el.EFOCALS[3], group_sizes=[F, 600 - F], caterpillar_at=1)
    inp = el.with_cond(inp, kind)
    assert inp["focal"].size == F and inp["cond"].size == {"plain": 600 - F, "same": F, "empty": 0}[kind]
    hnum, _ = _check_single(tmp_path, inp, el.EPOCHS, el.EFOCALS[3])
    assert (hnum != 0).any()


@MODES
def test_s4_more_trees_than_workgroups(ancient, tmp_path, monkeypatch):
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    T = 1100
    assert T > el.KMAXGRID == el.slab_grid(T, 2 * 2 * el.EPOCHS.size * 2)
    inp = el.dyadic_input(400, 8, T, 2, ancient, num_blocks=5)
    hnum, _ = _check_single(tmp_path, inp, el.EPOCHS, el.EFOCALS[2], model=True)
    assert (hnum != 0).any(axis=(1, 2, 3)).all()


def test_s5_grid_capped_by_the_slab_limit(tmp_path, monkeypatch):
    """G = 128 on a 31-epoch grid: 2 GiB of slabs hold fewer workgroups than there are trees."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    T, G = 70, 128
    assert el.slab_grid(T, 2 * 2 * el.EPOCHS31.size * G) < T
    inp = el.dyadic_input(500, 130, T, G, False, epochs=el.EPOCHS31, caterpillar_at=1)
    hnum, _ = _check_single(tmp_path, inp, el.EPOCHS31, el.EFOCALS[2])
    assert (hnum != 0).any()


S6_BLOCKS = {"six_blocks": (np.repeat(np.arange(6), [4, 1, 9, 2, 15, 10]), 6), "gaps": (np.repeat([0, 2, 5], [7, 1, 9]), 7)}


@MODES
@pytest.mark.parametrize("layout, chunk", [("six_blocks", "1"), ("six_blocks", "3"), ("gaps", "3")])
def test_s6_small_chunks(layout, chunk, ancient, tmp_path, monkeypatch):
    """Chunks of one and of three trees through the walker's two slots: blocks across chunks, chunks across blocks, block
    indices without a tree; against the unchunked host twin."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    blocks, nb = S6_BLOCKS[layout]
    inp = el.dyadic_input(600, 24, blocks.size, 4, ancient, blocks=blocks, num_blocks=nb, caterpillar_at=3)
    hnum, hden = _check_single(tmp_path, inp, el.EPOCHS, el.EFOCALS[2], env={"COLATE_CONDCOAL_CHUNK_TREES": chunk}, model=True)
    present = np.isin(np.arange(nb), blocks)
    assert (hnum[present] != 0).any(axis=(1, 2, 3)).all()
    assert not hnum[~present].any() and not hden[~present].any()


def _check_pairs(tmp_path, inp, fg, cg, epochs, efocal, env=None):
    """The pairs kernel against the single kernel pair by pair (one child) and against the host twin (unchunked)."""
    num, den, snum, sden = pl.in_child(tmp_path, inp, fg, cg, epochs, efocal, device=True, timeout=2 * CHILD_S, env=env)
    assert (num != 0).any(axis=tuple(range(1, num.ndim))).all()
    assert el.same_bits(num, snum)
    assert el.same_bits(den, sden)
    kw = {k: v for k, v in inp.items() if k not in ("focal", "cond")}
    hnum, hden = colate_amd.condcoal_accumulate_pairs(focal_group=fg, cond_group=cg, epochs=epochs, epochs_focal=efocal,
                                                      device=False, **kw)
    assert el.same_bits(num, hnum)
    assert el.same_bits(den, hden)


@MODES
def test_p1_units_and_batches(ancient, tmp_path, monkeypatch):
    """Two pairs in a unit of exactly 256 items, pairs of 300 and 257 focal haplotypes as units of their own and continued
    over batches, a pair of 256 (p1_input asserts the layout)."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    inp = el.p1_input(ancient)
    fg, cg = el.P1_PAIRS
    _check_pairs(tmp_path, inp, fg, cg, el.EPOCHS, el.EFOCALS[3])


P2_BLOCKS = np.repeat([0, 1, 3, 4, 5, 8, 9, 10, 12, 13, 14, 17], [3, 1, 4, 2, 1, 5, 2, 3, 1, 4, 2, 2])


@MODES
@pytest.mark.parametrize("chunk", [None, "1"], ids=["one_chunk", "chunks_of_1"])
def test_p2_block_closes(chunk, ancient, tmp_path, monkeypatch):
    """Eleven blocks close inside one chunk: it is launched in pieces that close four each, through both buffers of closed
    blocks; and every tree a chunk of its own."""
    monkeypatch.delenv("COLATE_CONDCOAL_CHUNK_TREES", raising=False)
    assert P2_BLOCKS.size == 30 and np.unique(P2_BLOCKS).size == 12
    assert len(el.launch_pieces(P2_BLOCKS)) >= 3
    inp = el.dyadic_input(700, 24, 30, 3, ancient, efocal=el.EFOCALS[3], blocks=P2_BLOCKS, num_blocks=19, shuffled_at=4)
    fg = [a for a in range(3) for _ in range(3)]
    cg = [b for _ in range(3) for b in range(3)]
    _check_pairs(tmp_path, inp, fg, cg, el.EPOCHS, el.EFOCALS[3], env={"COLATE_CONDCOAL_CHUNK_TREES": chunk} if chunk else None)
