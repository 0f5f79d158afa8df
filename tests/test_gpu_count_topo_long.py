"""The count_topo kernels past the fourth tile of a block: the four device calls on the long case of count_topo_long_lib.py -- blocks
of 5 tiles + 2 words from a word that is no multiple of the tile, of exactly one tile, of one tile + one word and of exactly 10
tiles, a chromosome of 17 tiles + 4 words, ranks and cells above 2^16, two empty chromosomes at the genome's end -- against the
host twins and the independent models in every bit and integer, at four block sizes, and in two chunks of four and three triples.
tests/test_count_topo_long_cpu.py checks that the case is what it says and the twins against the models."""
import os

import numpy as np
import pytest

import colate_amd
import count_topo_expected_lib as xl
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_long_lib as ll
import count_topo_profile_lib as pl

pytestmark = pytest.mark.gpu


def test_samples_on_the_long_case_equal_twin_and_model_in_every_bit():
    """topo_draw_kernel over a chromosome of 18 tiles behind one of 3 rows: waves 0 and 1 store five tiles each, wave 3 four; rank =
    row beyond 2^16 in the triple whose every row qualifies; the plane kernel's chromosome search with two empty chromosomes last"""
    got = tl.topo(ll.long_case(), device=True)
    tl.assert_same(got, ll.twin_planes())
    tl.assert_same(got, ll.modelled_planes())
    assert colate_amd.topo_samples_chunks() == 1
    assert got[3][ll.ALL_ROWS] == ll.long_case()["rows"].size > 65535


def test_samples_on_the_profiles_long_case_equal_twin_and_model_in_every_bit():
    """5 TILE + 3 rows behind a chromosome of 3, with the triples and the injected uniforms of count_topo_lib: the profile's case,
    whose planes no GPU test had asked for"""
    c = pl.cases()["long"]
    got = tl.topo(c, device=True)
    tl.assert_same(got, pl.twin_planes("long"))
    tl.assert_same(got, tl.model(c))
    assert colate_amd.topo_samples_chunks() == 1


@pytest.mark.parametrize("E", (1, 1024))
def test_profile_on_the_long_case_equals_twin_and_model(E):
    """topo_profile_kernel<Chromosomes> over 18 tiles; at E = 1 one cell of the workgroup's histogram passes 2^16"""
    got = pl.profile(ll.long_case(), pl.EPOCHS[E], device=True)
    pl.assert_same(got, ll.twin_profile(E))
    pl.assert_same(got, ll.modelled_profile(E))
    assert colate_amd.topo_profile_chunks() == 1


@pytest.mark.parametrize("E", (1, 11, 1024))
def test_blocks_longer_than_a_round_of_the_waves(E):
    """topo_count_kernel<Blocks>, topo_profile_kernel<Blocks> and topo_block_expected_kernel at B bases per block: a segment from word
    3 over 5 tiles + 2 words (wave 0 takes a second tile, the partial last one is wave 1's, 6 trips of the count kernel's lanes), one
    of exactly 64 words from inside word 324, one of 65 words, one of exactly 10 tiles from inside word 452, a block without a row;
    ranks carried through tiles without a set bit; words whose only set bit is the neighbouring block's"""
    c, ep = ll.long_case(), pl.EPOCHS[E]
    blocks = jl.profile_blocks(c, ep, ll.B, device=True)
    assert colate_amd.topo_profile_blocks_chunks() == 1
    expected = xl.expected(c, ep, ll.B, device=True)
    assert colate_amd.topo_expected_blocks_chunks() == 1
    ll.assert_blocks_same(blocks, ll.twin_blocks(E))
    ll.assert_blocks_same(blocks, ll.modelled_blocks(E))
    xl.assert_same(expected, ll.twin_expected(E))
    xl.assert_equals_model(expected[1], ll.modelled_expected(E))
    ll.assert_blocks_of_the_case(blocks, expected, pl.profile(c, ep, device=True))  # the block sums are the device's own profile


@pytest.mark.parametrize("nbpb,E", [(ll.NBPB_WHOLE, 1), (ll.NBPB_WHOLE, 11), (ll.NBPB_PAIRS, 11), (1, 11)])
def test_other_block_sizes_equal_the_twin_in_every_integer(nbpb, E):
    """1000 B bases: one block per chromosome, a segment of 17 tiles + 4 words from word 0, and at E = 1 a cell of 69 888.  2 B: the
    blocks merge in pairs, the first a segment of 6 tiles from word 0 that ends inside word 324.  One base per block: more than 6000
    blocks, within kMaxTopoBlocks = 65535 since the positions stay below 6 B; a block is the rows at one position."""
    c, ep = ll.long_case(), pl.EPOCHS[E]
    nb = int(colate_amd.topo_blocks(c["row_off"], c["rows"], nbpb)[-1])
    assert nb == {ll.NBPB_WHOLE: 4, ll.NBPB_PAIRS: 6}.get(nbpb, nb) and nb <= 65535
    blocks = jl.profile_blocks(c, ep, nbpb, device=True)
    expected = xl.expected(c, ep, nbpb, device=True)
    ll.assert_blocks_same(blocks, ll.twin_blocks(E, nbpb))
    xl.assert_same(expected, ll.twin_expected(E, nbpb))
    assert (expected[1][..., 2] == blocks[1][..., 2]).all() and blocks[1].shape[1] == nb
    if E == 1 and nbpb == ll.NBPB_WHOLE:
        assert blocks[1][ll.ALL_ROWS, :, 0, 2].tolist() == [ll.N0, ll.N1, 0, 0]
    if nbpb == 1:
        assert nb > 6000
        assert (blocks[1][ll.ALL_ROWS, :, :, 2].sum(axis=1) == np.bincount(jl.row_blocks(c, 1, blocks[0]), minlength=nb)).all()


def budget_of(value, run):
    """run() under COLATE_TOPO_BUDGET = value (None: the default), the caller's setting restored"""
    old = os.environ.pop("COLATE_TOPO_BUDGET", None)
    try:
        if value is not None:
            os.environ["COLATE_TOPO_BUDGET"] = str(value)
        return run()
    finally:
        os.environ.pop("COLATE_TOPO_BUDGET", None)
        if old is not None:
            os.environ["COLATE_TOPO_BUDGET"] = old


def test_four_triples_per_chunk_of_samples_change_no_bit():
    """seven triples in chunks of four: the second chunk has p0 = 4 and j = 0 .. 2, so triples[p0 + j], base[(p0 + j) C + c] and the
    planes at j words meet with both above 0"""
    c = ll.long_case()
    words = int(ll.twin_planes()[0][-1])

    def chunked():
        got = tl.topo(c, device=True)
        return got, colate_amd.topo_samples_chunks()

    one, chunks = budget_of(None, chunked)
    assert chunks == 1
    two, chunks = budget_of(4 * 16 * words + 5, chunked)
    assert chunks == 2
    tl.assert_same(two, one)
    tl.assert_same(two, ll.twin_planes())


def test_four_triples_per_chunk_of_the_block_calls_change_no_integer():
    """the same for topo_profile_kernel<Blocks> (12 E nb bytes per triple) and topo_block_expected_kernel (24 E nb): part + blockIdx.x
    * 3 E of the second chunk's triples"""
    c, E = ll.long_case(), 11
    ep, nb = pl.EPOCHS[E], int(ll.twin_blocks(E)[0][-1])

    def profiled():
        got = jl.profile_blocks(c, ep, ll.B, device=True)
        return got, colate_amd.topo_profile_blocks_chunks()

    def expected():
        got = xl.expected(c, ep, ll.B, device=True)
        return got, colate_amd.topo_expected_blocks_chunks()

    one, chunks = budget_of(None, profiled)
    assert chunks == 1
    two, chunks = budget_of(4 * 12 * E * nb + 5, profiled)
    assert chunks == 2
    ll.assert_blocks_same(two, one)
    ll.assert_blocks_same(two, ll.twin_blocks(E))
    one, chunks = budget_of(None, expected)
    assert chunks == 1
    two, chunks = budget_of(4 * 24 * E * nb + 5, expected)
    assert chunks == 2
    xl.assert_same(two, one)
    xl.assert_same(two, ll.twin_expected(E))
