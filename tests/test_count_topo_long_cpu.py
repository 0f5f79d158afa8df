"""The long case of count_topo_long_lib.py without a device: the case is what its table says -- every block's first word, words,
first and last bit, and tiles, from colate_topo_blocks and the rows' positions --, and the four host twins equal their independent
models on it in every integer, so that tests/test_gpu_count_topo_long.py asks the device for integers that are known to be right."""
import numpy as np
import pytest

import colate_amd
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_long_lib as ll
import count_topo_profile_lib as pl
import count_topo_expected_lib as xl

TILE_WORDS = tl.TILE // 64
WAVES = 4  # of a draw workgroup (kDrawWaves)


def test_the_case_is_what_the_table_says():
    c = ll.long_case()
    row_off = c["row_off"]
    assert np.diff(row_off).tolist() == [3, ll.N1, 0, 0] and ll.N1 == 69888 and c["rows"].size == 69891
    # the long chromosome starts at word 1; 1092 words = 17 tiles + 4 words
    assert ll.twin_planes()[0].tolist() == [0, 1, 1093, 1093, 1093] and ll.modelled_planes()[0].tolist() == [0, 1, 1093, 1093, 1093]
    assert divmod(1092, TILE_WORDS) == (17, 4)
    blk_off = colate_amd.topo_blocks(row_off, c["rows"], ll.B)
    assert blk_off.tolist() == [0, 1, 7, 8, 9] and (blk_off == jl.blocks_model(row_off, c["rows"]["pos"], ll.B)).all()
    pos = c["rows"]["pos"].astype(np.int64)
    assert ((pos - 1) % ll.B < ll.B - 1).all() and (pos % ll.B != 0).all()  # strictly inside the block
    blk = jl.row_blocks(c, ll.B, blk_off)
    assert (np.diff(blk) >= 0).all()
    q = ll.qualifying(c)
    for k in range(6):
        at = np.nonzero(blk == ll.LONG_BLOCK0 + k)[0] - ll.N0  # rows of the long chromosome
        assert (q[ll.SPARSE_Q][ll.N0 + at].sum(), q[ll.NEIGHBOUR_Q][ll.N0 + at].sum()) == (ll.SPARSE_PER_BLOCK[k], ll.NEIGHBOUR_PER_BLOCK[k]), k
        if k == 3:
            assert at.size == 0  # a gap in the positions
            continue
        first, end = int(at[0]), int(at[-1]) + 1
        assert (first, end) == ll.BLOCK_ROWS[k] and at.size == end - first
        w_first, w_end = first >> 6, (end + 63) >> 6
        tiles = -(-(w_end - w_first) // TILE_WORDS)
        assert (w_first, w_end - w_first, first & 63, end & 63, tiles) == ll.GEOMETRY[k], k
    assert [np.count_nonzero(blk == ll.LONG_BLOCK0 + k) for k in range(6)] == [229, 20550, 4053, 0, 4140, 40916]
    # block 1: no multiple of the tile in front, more than one round of the waves, a partial last tile that is wave 1's
    w_first, words = ll.GEOMETRY[1][:2]
    assert w_first % TILE_WORDS != 0 and words == 5 * TILE_WORDS + 2 and 5 % WAVES == 1 and -(-words // 64) == 6
    # block 5: the tile loop ends on tile0 == w_end, every wave has made a second trip and waves 0 and 1 a third
    assert ll.GEOMETRY[5][1] == 10 * TILE_WORDS and ll.GEOMETRY[5][0] + ll.GEOMETRY[5][1] == 1092
    # SPARSE in block 1: segment tiles 0, 1, 4 and 5 hold its rows and tiles 2 and 3 none, so a rank is carried through whole tiles
    sparse = np.array(ll.SPARSE_ROWS)
    assert sorted(set(((sparse[(sparse >= 229) & (sparse < 20779)] >> 6) - 3) // TILE_WORDS)) == [0, 1, 4, 5]
    assert np.nonzero(q[ll.SPARSE_Q])[0].tolist() == (ll.N0 + sparse).tolist()
    assert np.nonzero(q[ll.NEIGHBOUR_Q])[0].tolist() == [ll.N0 + r for r in ll.NEIGHBOUR_ROWS]
    # NEIGHBOUR's rows lie in the first word of block 1, the last word of block 1 and the last word of block 4, and in none of the two
    assert [r >> 6 for r in ll.NEIGHBOUR_ROWS] == [3, 324, 452] and ll.GEOMETRY[1][0] == 3 and 3 + 322 - 1 == 324 and 388 + 65 - 1 == 452
    assert not q[ll.NO_ROW].any() and q[ll.ALL_ROWS].all()
    for p in (4, 5, 6):  # the random triples: about 0.5 * 0.5 * 0.6 of the rows
        assert 0.1 < q[p].mean() < 0.2
    assert c["uniforms"].size == 2 * c["rows"].size  # the stream is exactly as long as the longest triple needs
    # the two other block sizes of the GPU tests: one block per chromosome; pairs of blocks, the first from word 0 into word 324
    assert np.diff(colate_amd.topo_blocks(row_off, c["rows"], ll.NBPB_WHOLE)).tolist() == [1, 1, 1, 1]
    pairs = jl.row_blocks(c, ll.NBPB_PAIRS, colate_amd.topo_blocks(row_off, c["rows"], ll.NBPB_PAIRS))
    at = np.nonzero(pairs == 1)[0] - ll.N0
    assert (int(at[0]), int(at[-1]) + 1) == (0, 20779) and -(-((20779 + 63) >> 6) // TILE_WORDS) == 6 and 20779 & 63 != 0
    assert 6000 < int(colate_amd.topo_blocks(row_off, c["rows"], 1)[-1]) <= 65535  # one base per block is within kMaxTopoBlocks


def test_samples_twin_equals_the_model_in_every_bit():
    got, want = ll.twin_planes(), ll.modelled_planes()
    tl.assert_same(got, want)
    _, plus, minus, draws = got
    n = ll.long_case()["rows"].size
    assert draws[ll.ALL_ROWS] == n and n > 65535  # rank = row: ranks above 2^16
    assert draws.tolist()[:4] == [n, 0, len(ll.SPARSE_ROWS), len(ll.NEIGHBOUR_ROWS)] and (draws[4:] > 5000).all()
    assert not plus[ll.NO_ROW].any() and not minus[ll.NO_ROW].any() and (plus & minus == 0).all()
    for p in (ll.ALL_ROWS, 4, 5, 6):  # both signs in the last tile of the long chromosome: the draws reach its end
        assert plus[p, -4:].any() and minus[p, -4:].any() and plus[p, 1:65].any() and minus[p, 1:65].any(), p


@pytest.mark.parametrize("E", (1, 11, 1024))
def test_profile_twin_equals_the_model_in_every_integer(E):
    got = ll.twin_profile(E)
    pl.assert_same(got, ll.modelled_profile(E))
    pl.assert_invariants(ll.long_case(), got, ll.modelled_planes())
    if E == 1:
        assert got[0][ll.ALL_ROWS, 0, 2] == 69891  # one cell above 65 535


@pytest.mark.parametrize("E", (1, 11, 1024))
def test_block_twins_equal_their_models_in_every_integer(E):
    c = ll.long_case()
    blocks, expected = ll.twin_blocks(E), ll.twin_expected(E)
    ll.assert_blocks_same(blocks, ll.modelled_blocks(E))
    assert expected[1].shape == (len(ll.TRIPLES), 9, E, 3)
    xl.assert_equals_model(expected[1], ll.modelled_expected(E))
    assert (expected[0] == jl.blocks_model(c["row_off"], c["rows"]["pos"], ll.B)).all()
    ll.assert_blocks_of_the_case(blocks, expected, ll.twin_profile(E))  # the sums over the blocks; column 2 of both
    if E == 1:
        assert blocks[1][ll.ALL_ROWS, ll.LONG_BLOCK0 + 5, 0, 2] == 40916
    assert (expected[1][ll.ALL_ROWS, :, :, :2] % xl.ONE).any()  # not fixed rows alone: the quotients are formed
