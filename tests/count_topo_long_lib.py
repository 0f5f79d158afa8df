"""What tests/test_count_topo_long_cpu.py and tests/test_gpu_count_topo_long.py share: one case whose blocks are longer than the four
tiles a draw workgroup's waves take in one round, so that every tile loop of count_topo_kernel.hip makes a second trip, wave 3 owns a
tile, segments begin at a word that is no multiple of the tile and ranks and histogram cells pass 2^16; a numpy model of the profile
per block that takes no integer from the C++; and the case's results on the host, each computed once.  The helpers of
count_topo_lib.py, count_topo_profile_lib.py, count_topo_jackknife_lib.py and count_topo_expected_lib.py are imported, not changed."""
import functools

import numpy as np

import colate_amd
import count_topo_expected_lib as xl
import count_topo_jackknife_lib as jl
import count_topo_lib as tl
import count_topo_profile_lib as pl

F32 = np.float32
T = tl.TILE
B = 1000                   # bases per block
N0 = 3                     # the short chromosome in front: the long one starts at plane word 1
N1 = 452 * 64 + 10 * T     # the long chromosome: 69 888 rows, 1092 words = 17 tiles + 4 words
# the long chromosome's blocks as [first, end) of its own rows; block 3 holds none
BLOCK_ROWS = {0: (0, 229), 1: (229, 229 + 5 * T + 70), 2: (20779, 24832), 4: (24832, 28972), 5: (28972, N1)}
# per block: first >> 6, words, first & 63, end & 63, tiles of the segment
GEOMETRY = {0: (0, 4, 0, 37, 1),       # ends inside word 3
            1: (3, 322, 37, 43, 6),    # a first word that is no multiple of 64; 5 tiles + 2 words: wave 0 takes segment tiles 0 and 4
            2: (324, 64, 43, 0, 1),    # shares word 324 with block 1; exactly one tile; ends on a word boundary
            4: (388, 65, 0, 44, 2),    # begins on a word boundary; a second tile of one word
            5: (452, 640, 44, 0, 10)}  # begins inside word 452; exactly 10 tiles: the loop ends on tile0 == w_end
RANDOM0, RANDOM1, RANDOM2, FULL, FULL2, EMPTY, SPARSE, NEIGHBOUR = range(8)
TRIPLES = [(FULL, FULL, FULL2),          # (cond, target, reference) every row qualifies: rank = row, above 65 535
           (FULL, EMPTY, FULL2),         # no qualifying row
           (FULL, SPARSE, FULL2),        # a few rows: whole tiles without a set bit between consecutive ranks
           (FULL, NEIGHBOUR, FULL2),     # raw Q != 0 in the first or last word of blocks 1 and 4, nothing of their own after the mask
           (RANDOM0, RANDOM1, RANDOM2),
           (RANDOM1, RANDOM2, RANDOM0),
           (RANDOM2, RANDOM0, RANDOM1)]
ALL_ROWS, NO_ROW, SPARSE_Q, NEIGHBOUR_Q = range(4)  # triples by what they are for
# rows of the long chromosome at which SPARSE hits: the last of block 0; the first, second and last of block 1; the last bit of
# block 1's segment tile 0 and the first of its tile 1; the first row of its tile 4; the first and last rows of blocks 2, 4 and 5
SPARSE_ROWS = (228, 229, 230, 3 * 64 + T - 1, 3 * 64 + T, (3 + 4 * 64) * 64, 20778, 20779, 24831, 24832, 28971, 28972, N1 - 1)
SPARSE_PER_BLOCK = [1, 6, 2, 0, 2, 2]
# ... and NEIGHBOUR: the last row of block 0 (bit 36 of word 3, block 1's first), the first of block 2 (bit 43 of word 324, block 1's
# last) and the first of block 5 (bit 44 of word 452, block 4's last)
NEIGHBOUR_ROWS = (228, 20779, 28972)
NEIGHBOUR_PER_BLOCK = [1, 0, 1, 0, 0, 1]
LONG_BLOCK0 = 1  # the global block of the long chromosome's block 0 at B bases per block: the short chromosome owns one block
NBPB_WHOLE, NBPB_PAIRS = 1000 * B, 2 * B  # one block per chromosome: 17 tiles + 4 words from word 0; blocks merged in pairs


@functools.lru_cache(maxsize=None)
def long_case():
    """Four chromosomes of 3, N1, 0 and 0 rows.  Positions as count_topo_jackknife_lib.edge_case places them: ascending, strictly inside
    the block.  Ages and counts as there.  FULL and FULL2 hit and qualify everywhere, EMPTY never hits, SPARSE and NEIGHBOUR hit at the
    rows above, three random samples hit at about half the rows and qualify at about 60 %.  The stream is exactly 2 n uniforms."""
    assert T == 4096
    rng = np.random.default_rng(97)
    n = N0 + N1
    pos = np.zeros(n, dtype=np.int64)
    pos[:N0] = [100, 200, 300]
    for k, (a, b) in BLOCK_ROWS.items():
        m = b - a
        pos[N0 + a:N0 + b] = k * B + 1 + (np.arange(m) * (B - 2)) // m  # ascending within (k B, (k + 1) B), B excluded
    assert (np.diff(pos[N0:]) >= 0).all()
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"] = pos
    rows["age_begin"] = rng.uniform(1.0, 2000.0, n).astype(F32)
    rows["age_end"] = rows["age_begin"] * rng.uniform(1.0, 2.0, n).astype(F32)
    S = 8
    idx = np.zeros((S, n), dtype=colate_amd.WALK_IDX)
    idx["DAF"], idx["AAF"] = rng.integers(0, 4, (S, n)), rng.integers(1, 4, (S, n))
    cidx = idx.copy()
    cidx["DAF"] = rng.integers(1, 5, (S, n))
    for s in (RANDOM0, RANDOM1, RANDOM2):
        hit, qual = rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.6
        idx["DAF"][s], idx["AAF"][s] = np.where(hit, idx["DAF"][s], 0), np.where(hit, idx["AAF"][s], 0)
        cidx["DAF"][s] = np.where(qual, cidx["DAF"][s], 0)
    idx["DAF"][EMPTY], idx["AAF"][EMPTY] = 0, 0
    for s, at in ((SPARSE, SPARSE_ROWS), (NEIGHBOUR, NEIGHBOUR_ROWS)):
        keep = np.zeros(n, dtype=bool)
        keep[N0 + np.array(at)] = True
        idx["DAF"][s], idx["AAF"][s] = np.where(keep, idx["DAF"][s], 0), np.where(keep, idx["AAF"][s], 0)
    return dict(row_off=np.array([0, N0, n, n, n], dtype=np.int64), rows=rows, idx=idx, cond_idx=cidx,
                triples=np.array(TRIPLES, dtype=colate_amd.TOPO_TRIPLE), uniforms=rng.uniform(size=2 * n))


def qualifying(c):
    """Q [P][rows] as booleans, by the rule of count_topo_lib.model"""
    hit = (c["idx"]["DAF"] | c["idx"]["AAF"]) != 0
    qual = c["cond_idx"]["DAF"] > 0
    return np.array([hit[int(t["target"])] & hit[int(t["reference"])] & qual[int(t["cond"])] for t in c["triples"]])


def blocks_model(c, epochs, nbpb, planes):
    """(blk_off, counts [P, nb, E, 3], draws) of a case in numpy: the plus and minus bits of `planes` (count_topo_lib.model's) and Q,
    binned by (count_topo_jackknife_lib.row_blocks, count_topo_profile_lib.age_epoch)"""
    _, plus, minus, draws = planes
    blk_off = jl.blocks_model(c["row_off"], c["rows"]["pos"], nbpb)
    nb, E = int(blk_off[-1]), len(epochs)
    cell = jl.row_blocks(c, nbpb, blk_off) * E + pl.age_epoch(c["rows"]["age_begin"], c["rows"]["age_end"], epochs)
    counts = np.zeros((len(c["triples"]), nb, E, 3), dtype=np.int64)
    for p, q in enumerate(qualifying(c)):
        for k, bits in enumerate((pl.unpack(plus[p], c["row_off"]), pl.unpack(minus[p], c["row_off"]), q)):
            counts[p, :, :, k] = np.bincount(cell[bits], minlength=nb * E).reshape(nb, E)
    return blk_off, counts, np.asarray(draws, dtype=np.int64)


# ------------------------------------------------------------------ the case's results on the host, each once; nobody writes to them
@functools.lru_cache(maxsize=None)
def modelled_planes():
    return tl.model(long_case())


@functools.lru_cache(maxsize=None)
def twin_planes():
    return tl.topo(long_case(), device=False)


@functools.lru_cache(maxsize=None)
def twin_profile(E):
    return pl.profile(long_case(), pl.EPOCHS[E], device=False)


@functools.lru_cache(maxsize=None)
def modelled_profile(E):
    return pl.model(long_case(), pl.EPOCHS[E], modelled_planes())


@functools.lru_cache(maxsize=None)
def twin_blocks(E, nbpb=B):
    return jl.profile_blocks(long_case(), pl.EPOCHS[E], nbpb, device=False)


@functools.lru_cache(maxsize=None)
def modelled_blocks(E, nbpb=B):
    return blocks_model(long_case(), pl.EPOCHS[E], nbpb, modelled_planes())


@functools.lru_cache(maxsize=None)
def twin_expected(E, nbpb=B):
    return xl.expected(long_case(), pl.EPOCHS[E], nbpb, device=False)


@functools.lru_cache(maxsize=None)
def modelled_expected(E, nbpb=B):
    return xl.model(long_case(), pl.EPOCHS[E], nbpb)


def assert_blocks_same(got, want):
    for name, x, y in zip(("blk_off", "counts", "draws"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, x.shape, y.shape, np.argwhere(x != y)[:8])


def assert_blocks_of_the_case(blocks, expected, whole):
    """what profile_blocks and expected_blocks at B bases per block owe each other and the case, in the outputs given: the sums over
    the blocks are `whole` (the profile of the same machine), the qualifying rows of both calls are the same, EMPTY's triple is all
    zero and so is NEIGHBOUR's block 1 -- and its block 4 --, whose first and last words hold a neighbour's bit only"""
    blk_off, counts, draws = blocks
    assert (counts.sum(axis=1) == whole[0]).all() and (draws == whole[1]).all()
    assert (blk_off == expected[0]).all() and (expected[1][..., 2] == counts[..., 2]).all()
    for x in (counts, expected[1]):
        assert not x[NO_ROW].any() and not x[NEIGHBOUR_Q, LONG_BLOCK0 + 1].any() and not x[NEIGHBOUR_Q, LONG_BLOCK0 + 4].any()
        assert x[ALL_ROWS, :, :, 2].sum(axis=1).tolist() == [N0, 229, 20550, 4053, 0, 4140, 40916, 0, 0]
        assert x[SPARSE_Q, :, :, 2].sum(axis=1).tolist() == [0] + SPARSE_PER_BLOCK + [0, 0]
        assert x[NEIGHBOUR_Q, :, :, 2].sum(axis=1).tolist() == [0] + NEIGHBOUR_PER_BLOCK + [0, 0]
