"""What the tests of colate_topo_expected_blocks and `Colate --mode count_topo --expected` share: the contract of csrc/count_topo.h
(the expected counts) restated in Python integers, the files of the command line printed from those integers, and the rows of
extreme counts used on both machines.  The cases are those of count_topo_jackknife_lib.py, which is imported, not changed."""
import functools

import numpy as np

import colate_amd
import count_topo_jackknife_lib as jl
import count_topo_profile_lib as pl
import topo_jackknife_model as jackknife_model

ONE = 1 << 30
EXTREME = (1, 32767, 65534, 65535)


def model(c, epochs, nbpb):
    """{(triple, block, epoch): [sum plus_fx, sum minus_fx, qualifying rows]} of a case, in Python integers: the contract, exact"""
    blk = jl.row_blocks(c, nbpb, jl.blocks_model(c["row_off"], c["rows"]["pos"], nbpb)).tolist()
    epoch = pl.age_epoch(c["rows"]["age_begin"], c["rows"]["age_end"], epochs).tolist()
    D, A, out = c["idx"]["DAF"].tolist(), c["idx"]["AAF"].tolist(), {}
    for p, (cond, t, r) in enumerate(c["triples"].tolist()):
        for g in np.nonzero(c["cond_idx"]["DAF"][cond] > 0)[0].tolist():
            nT, nR = D[t][g] + A[t][g], D[r][g] + A[r][g]
            if nT > 0 and nR > 0:
                cell = out.setdefault((p, blk[g], epoch[g]), [0, 0, 0])
                cell[0] += D[t][g] * A[r][g] * ONE // (nT * nR)
                cell[1] += A[t][g] * D[r][g] * ONE // (nT * nR)
                cell[2] += 1
    return out


def dense(cells, shape):
    """counts [P, nb, E, 3] int64 of the model's cells"""
    out = np.zeros(shape, dtype=np.int64)
    for k, v in cells.items():
        out[k] = v
    return out


def assert_equals_model(counts, cells):
    """counts [P, nb, E, 3] hold the model's cells and nothing else: every listed cell equal, the totals equal, none negative"""
    assert counts.dtype == np.int64 and (counts >= 0).all()
    at = np.array(list(cells), dtype=np.int64).reshape(-1, 3)
    want = np.array(list(cells.values()), dtype=np.int64).reshape(-1, 3)
    got = counts[at[:, 0], at[:, 1], at[:, 2]]
    assert (got == want).all(), (at[(got != want).any(axis=1)][:8], got[(got != want).any(axis=1)][:8], want[(got != want).any(axis=1)][:8])
    for k in range(3):
        assert int(counts[..., k].sum()) == sum(v[k] for v in cells.values())


def expected(c, epochs, nbpb, device):
    return colate_amd.topo_expected_blocks(c["row_off"], c["rows"], c["idx"], c["cond_idx"], c["triples"], epochs, nbpb, device=device)


def assert_same(got, want):
    for name, x, y in zip(("blk_off", "counts"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, x.shape, y.shape, np.argwhere(x != y)[:8])


def fixed(x):
    """a fixed-point sum as the files print it"""
    return "%.6f" % (float(int(x)) * 2.0 ** -30)


def files(names, printed_epochs, counts):
    """(PREFIX.expected.txt, PREFIX.expected.jackknife.txt) from counts [P][nb][E][3] as nested lists of Python integers: the sums over
    the blocks printed %.6f of sum * 2^-30, the statistics of topo_jackknife_model on the integers as they are"""
    table, jk = [], []
    for name, blocks in zip(names, counts):
        E = len(blocks[0])
        per_epoch = [[sum(b[e][k] for b in blocks) for k in range(3)] for e in range(E)]
        table += ["%s %s %s %s %d" % (name, printed_epochs[e], fixed(x[0]), fixed(x[1]), x[2]) for e, x in enumerate(per_epoch)]
        stats, used = jackknife_model.jackknife(blocks)
        total = [sum(x[k] for x in per_epoch) for k in range(2)]
        for cell in range(E + 1):
            x = per_epoch[cell] if cell < E else total
            jk.append(" ".join([name, printed_epochs[cell] if cell < E else "all", fixed(x[0]), fixed(x[1]), str(used[cell])] +
                               [jackknife_model.number(v) for v in stats[cell]]))
    return "".join(line + "\n" for line in table), "".join(line + "\n" for line in jk)


@functools.lru_cache(maxsize=None)
def extreme_case():
    """Every combination of the counts 1, 32767, 65534 and 65535 as (DAF, AAF) of a target and of a reference, 256 rows laid from
    row 40 on across the boundaries of four words; one triple, every row qualifying; three blocks at 400 bases per block, whose boundaries cut the words"""
    combos = [(a, b, c, d) for a in EXTREME for b in EXTREME for c in EXTREME for d in EXTREME]
    n = 40 + len(combos) + 5
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"] = 1 + 3 * np.arange(n)
    rows["age_begin"], rows["age_end"] = 10.0 + np.arange(n) % 7, 20.0 + np.arange(n) % 5
    idx = np.zeros((3, n), dtype=colate_amd.WALK_IDX)
    idx["DAF"], idx["AAF"] = 1, 1
    for k, (a, b, c, d) in enumerate(combos):
        idx["DAF"][1, 40 + k], idx["AAF"][1, 40 + k], idx["DAF"][2, 40 + k], idx["AAF"][2, 40 + k] = a, b, c, d
    return dict(row_off=np.array([0, n], dtype=np.int64), rows=rows, idx=idx, cond_idx=idx.copy(),
                triples=np.array([(0, 1, 2)], dtype=colate_amd.TOPO_TRIPLE)), combos
