"""What the tests of colate_topo_blocks, colate_topo_profile_blocks and `Colate --mode count_topo --jackknife` share: the blocks of
csrc/count_topo.h restated in three lines, the fixture tests/golden/count_topo read and indexed here by the rules of the header
(independent of the C++ loader) with the reference's own lines binned per (block, epoch), and the edge rows used on the GPU.  The
helpers of count_topo_lib.py and count_topo_profile_lib.py are imported, not changed."""
import functools
import gzip
import json
import os
import struct

import numpy as np

import colate_amd
import count_topo_lib as tl
import count_topo_profile_lib as pl

F32 = np.float32
NBPB = (30_000_000, 5_000_000, 100_000)  # the command line's default; several blocks per chromosome; mostly one row or none per block
BINS = "3,7,0.2"                         # 23 epochs at 28 years per generation


def blocks_model(row_off, pos, nbpb):
    """blk_off of the contract: k(pos) = (pos - 1) // nbpb above 0, else 0; a chromosome owns k(its last row) + 1 blocks, 1 without a row"""
    k = lambda p: (int(p) - 1) // nbpb if p > 0 else 0  # noqa: E731
    own = [k(pos[row_off[c + 1] - 1]) + 1 if row_off[c + 1] > row_off[c] else 1 for c in range(len(row_off) - 1)]
    return np.concatenate([[0], np.cumsum(own)]).astype(np.int32)


def row_blocks(c, nbpb, blk_off):
    """the global block of every row of a case"""
    pos = c["rows"]["pos"].astype(np.int64)
    chrom = np.searchsorted(c["row_off"], np.arange(pos.size), side="right") - 1
    return blk_off[chrom].astype(np.int64) + np.where(pos > 0, (pos - 1) // nbpb, 0)


def profile_blocks(c, epochs, nbpb, device):
    return colate_amd.topo_profile_blocks(c["row_off"], c["rows"], c["idx"], c["cond_idx"], c["triples"], c["uniforms"], epochs, nbpb, device=device)


def epochs_sets():
    """E = 1, the 23 epochs of 3,7,0.2 as the command line hands them over (epochs[0] below epochs[1]), and 1024"""
    e23, _ = colate_amd.epochs_from_bins(BINS)
    e23 = e23.copy()
    assert e23.size == 23
    if e23[0] >= e23[1]:
        e23[0] = e23[1] - 1.0
    return {1: np.array([0.0]), 23: e23, 1024: np.arange(1024) * 40.0}


# ------------------------------------------------------------------ the fixture, read and indexed here
def _open(path):
    return gzip.open(path + ".gz", "rb") if os.path.exists(path + ".gz") else open(path, "rb")


def _records(path):
    """[(chromosome name, bp, anc, der, AAF, DAF)] of a .colate.in file, in file order"""
    with _open(path) as f:
        raw = f.read()
    out, at = [], 0
    while at < len(raw):
        (n,) = struct.unpack_from("<i", raw, at)
        name = raw[at + 4:at + 4 + n].decode()
        bp, anc, der, aaf, daf = struct.unpack_from("<iccii", raw, at + 4 + n)
        out.append((name, bp, anc.decode(), der.decode(), aaf, daf))
        at += 4 + n + 14
    return out


@functools.lru_cache(maxsize=None)
def fixture_case():
    """tests/golden/count_topo as topo_profile_blocks takes it: the searched rows of the .mut files (the filter of the header), per
    sample the walk index -- the counts of the record at the row's lower bound where its position and alleles are the row's -- and
    the cond index -- the counts of that record whatever it is; behind the chromosome's last record the next one of the file, or the
    file's last --, the triples of case.json in its order, and the stream of std::mt19937 on its seed.  Also: meta, chroms, and per
    row the printed ages."""
    d = tl.FIXTURE
    meta = json.load(open(os.path.join(d, "case.json")))
    chroms = open(os.path.join(d, "chr.txt")).read().split()
    pos, begin, end, alleles, row_off = [], [], [], [], [0]
    for ch in chroms:
        with _open(os.path.join(d, f"P_chr{ch}.mut")) as f:
            for line in f.read().decode().splitlines()[1:]:
                x = line.split(";")
                b, e = F32(x[8]), F32(x[9])
                al = x[10].split("/")
                if int(x[7]) == 0 and len(x[5].split()) == 1 and b <= e and len(al) == 2 and all(len(a) == 1 and a in "ACGT01" for a in al):
                    pos.append(int(x[1])), begin.append(b), end.append(e), alleles.append((al[0], al[1]))
        row_off.append(len(pos))
    n = len(pos)
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"], rows["age_begin"], rows["age_end"] = pos, begin, end
    files = [s.split()[1] for s in meta["samples"]]
    names = [s.split()[0] for s in meta["samples"]]
    idx, cidx = np.zeros((len(files), n), dtype=colate_amd.WALK_IDX), np.zeros((len(files), n), dtype=colate_amd.WALK_IDX)
    for s, fn in enumerate(files):
        R = _records(os.path.join(d, fn))
        for ci, ch in enumerate(chroms):
            run = [k for k, r in enumerate(R) if r[0] == ch]
            assert run and run == list(range(run[0], run[-1] + 1))
            b, e = run[0], run[-1] + 1
            bps = np.array([R[k][1] for k in range(b, e)], dtype=np.int64)
            for g in range(row_off[ci], row_off[ci + 1]):
                k = b + int(np.searchsorted(bps, pos[g], side="left"))
                if k < e and R[k][1] == pos[g] and (R[k][2], R[k][3]) == alleles[g]:
                    idx["DAF"][s, g], idx["AAF"][s, g] = R[k][5], R[k][4]
                at = R[k] if k < e else R[e] if e < len(R) else R[-1]
                cidx["DAF"][s, g], cidx["AAF"][s, g] = at[5], at[4]
    triples = np.array([tuple(names.index(x) for x in t["names"]) for t in meta["triples"]], dtype=colate_amd.TOPO_TRIPLE)
    case = dict(row_off=np.array(row_off, dtype=np.int64), rows=rows, idx=idx, cond_idx=cidx, triples=triples,
                uniforms=tl.mt_uniforms(int(meta["seed"]), 2 * n))
    printed = np.array(["%g %g" % (float(b), float(e)) for b, e in zip(begin, end)])
    return case, meta, chroms, printed


def reference_lines():
    """[(triple, global row)] with its sign, of every line of the reference's expected_*.txt: matched to its searched row by
    chromosome, position and printed ages as count_topo_profile_lib.reference_profile matches them -- unique in the floats that
    decide the epoch, and here also in the position, which decides the block"""
    case, meta, chroms, printed = fixture_case()
    rows, row_off = case["rows"], case["row_off"]
    out = []
    for p, t in enumerate(meta["triples"]):
        for line in open(os.path.join(tl.FIXTURE, t["output"])).read().splitlines():
            x = line.split(" ")
            ci = chroms.index(x[0])
            lo, hi = int(row_off[ci]), int(row_off[ci + 1])
            at = lo + np.nonzero((rows["pos"][lo:hi] == int(x[1])) & (printed[lo:hi] == x[2] + " " + x[3]))[0]
            floats = {(rows["age_begin"][i].tobytes(), rows["age_end"][i].tobytes()) for i in at}
            assert len(floats) == 1, (t["output"], line, at)
            out.append((p, int(at[0]), int(x[4])))
    return out


def reference_blocks(epochs, nbpb, blk_off):
    """{(triple, block, epoch, 0 for plus / 1 for minus): lines} of the reference's files"""
    case = fixture_case()[0]
    blk = row_blocks(case, nbpb, blk_off)
    epoch = pl.age_epoch(case["rows"]["age_begin"], case["rows"]["age_end"], epochs)
    want = {}
    for p, g, sign in reference_lines():
        key = (p, int(blk[g]), int(epoch[g]), 0 if sign > 0 else 1)
        want[key] = want.get(key, 0) + 1
    return want


def assert_equals_reference(counts, want):
    """plus and minus of counts [P, nb, E, 3] are `want` and nothing else: every listed cell equal and the totals equal, none negative"""
    assert (counts >= 0).all()
    for which in (0, 1):
        cells = {k[:3]: v for k, v in want.items() if k[3] == which}
        assert int(counts[..., which].sum()) == sum(cells.values())
        at = np.array(list(cells), dtype=np.int64)
        got = counts[at[:, 0], at[:, 1], at[:, 2], which]
        assert (got == np.array(list(cells.values()))).all(), (which, at[got != np.array(list(cells.values()))][:8])


# ------------------------------------------------------------------ the edge rows
B = 1000                   # bases per block of the edge case
N0 = 2 * tl.TILE + 64 + 3  # the main chromosome: two draw tiles, one word, a ragged tail
FULL, FULL2, EMPTY, SPARSE = range(4)
EDGE_TRIPLES = [(FULL, FULL, FULL2), (FULL, EMPTY, FULL2), (FULL, SPARSE, FULL2)]  # every row; no row; a few rows
SPARSE_ROWS = (37, 38, 63, 64, tl.TILE - 1, tl.TILE, tl.TILE + 1, N0 - 2, N0 - 1)
# the first row of every block of the main chromosome and the block it opens: inside a word (37 | 38), on a word boundary (63 | 64),
# one row before the tile boundary, on it and one row after it, a gap that leaves blocks 7 and 8 without a row, and a last block that
# holds the last row alone
FIRST_ROWS = {0: 0, 38: 1, 64: 2, tl.TILE - 1: 3, tl.TILE: 4, tl.TILE + 1: 5, 6000: 6, 7000: 9, N0 - 1: 10}


@functools.lru_cache(maxsize=None)
def edge_case():
    """Three chromosomes: N0 rows with the block boundaries of FIRST_ROWS placed by position at B bases per block, none, and one row.
    Row 63 lies on pos = 2 B, the last base of block 1, and row 64 on 2 B + 1, the first of block 2; rows 10 .. 12 share a position.
    FULL and FULL2 hit and qualify everywhere, EMPTY never hits, SPARSE hits at SPARSE_ROWS.  Positions stay below 12 000, so one
    base per block is within 65535 blocks."""
    assert tl.TILE == 4096
    rng = np.random.default_rng(91)
    n = N0 + 1
    first = sorted(FIRST_ROWS)
    pos = np.zeros(n, dtype=np.int64)
    for a, b in zip(first, first[1:] + [N0]):
        k, m = FIRST_ROWS[a], b - a
        pos[a:b] = k * B + 1 + (np.arange(m) * (B - 2)) // m  # ascending within (k B, (k + 1) B), B excluded
    pos[63], pos[10:13] = 2 * B, pos[10]
    assert pos[64] == 2 * B + 1 and (np.diff(pos[:N0]) >= 0).all()
    pos[N0] = 500  # the third chromosome's only row
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"] = pos
    rows["age_begin"] = rng.uniform(1.0, 2000.0, n).astype(F32)
    rows["age_end"] = rows["age_begin"] * rng.uniform(1.0, 2.0, n).astype(F32)
    idx = np.zeros((4, n), dtype=colate_amd.WALK_IDX)
    idx["DAF"], idx["AAF"] = rng.integers(0, 4, (4, n)), rng.integers(1, 4, (4, n))
    cidx = idx.copy()
    cidx["DAF"] = rng.integers(1, 5, (4, n))
    idx["DAF"][EMPTY], idx["AAF"][EMPTY] = 0, 0
    keep = np.zeros(n, dtype=bool)
    keep[list(SPARSE_ROWS)] = True
    idx["DAF"][SPARSE], idx["AAF"][SPARSE] = np.where(keep, idx["DAF"][SPARSE], 0), np.where(keep, idx["AAF"][SPARSE], 0)
    return dict(row_off=np.array([0, N0, N0, n], dtype=np.int64), rows=rows, idx=idx, cond_idx=cidx,
                triples=np.array(EDGE_TRIPLES, dtype=colate_amd.TOPO_TRIPLE), uniforms=rng.uniform(size=2 * n))


def regroup(fine, fine_off, fine_nbpb, coarse_off, coarse_nbpb):
    """counts [P, nb, E, 3] at fine_nbpb bases per block summed into the blocks of coarse_nbpb, a multiple of it: block k of a
    chromosome goes to block k * fine_nbpb // coarse_nbpb of the same chromosome"""
    assert coarse_nbpb % fine_nbpb == 0
    out = np.zeros((fine.shape[0], int(coarse_off[-1])) + fine.shape[2:], dtype=np.int64)
    for c in range(len(fine_off) - 1):
        for k in range(int(fine_off[c + 1] - fine_off[c])):
            out[:, int(coarse_off[c]) + k * fine_nbpb // coarse_nbpb] += fine[:, int(fine_off[c]) + k]
    return out
