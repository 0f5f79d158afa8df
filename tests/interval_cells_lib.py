"""What the tests of the interval cells (colate_interval_bin_thresholds, colate_interval_cells[_host], `Colate --mode
mut_interval --mut ...`) share: a Python restatement of the age bin, the ordered plain loop the tables are compared with, the
scripted record sets (the same ones for the host twin against the loop and for the device against the host twin), and the
CLI runners."""
import functools
import math
import os
import subprocess

import numpy as np

import colate_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")
BINS = 185
CELLS = BINS * (BINS + 1) // 2


def bin_restated(x):
    """age_bin_index(x, 10) of csrc/age_bins.hpp (coal.cpp:2265) for a float32 widened to double: max(0, (int)round(log(10 x) * 10)
    + 1), round = half away from zero, log(0) -> bin 0"""
    x = float(x)
    if x <= 0.0:
        return 0
    v = math.log(10.0 * x) * 10.0
    r = math.copysign(math.floor(abs(v) + 0.5), v)
    return max(0, int(r) + 1)


@functools.lru_cache(maxsize=None)
def thresholds():
    return colate_amd.interval_bin_thresholds()


@functools.lru_cache(maxsize=None)
def grid():
    return colate_amd.age_grid()


def bin_table(x):
    return int(np.searchsorted(thresholds(), np.float32(x), side="right"))


def age_in_bin(b):
    """a float32 age whose bin is b: 0 for bin 0, else the threshold itself"""
    return np.float32(0.0) if b == 0 else thresholds()[b - 1]


def cell_of_index(c):
    """(bb, be) of the triangular index c = be (be + 1) / 2 + bb"""
    be = 0
    while (be + 1) * (be + 2) // 2 <= c:
        be += 1
    return c - be * (be + 1) // 2, be


def loop_cells(begin, end, w_sh, w_ns, block, nb, order=None):
    """The contract the plain way: per (kind, bb, be) and block a sum from 0.0 over the records in order (`order`: another
    order of addition, to show that the order matters), every addition rounded; rows = cells positive in some block, sorted
    by kind, bb, be.  Returns (kinds, age_begin, age_end, tables, dropped) like colate_amd.interval_cells."""
    cells, dropped = {}, 0
    idx = range(len(begin)) if order is None else order
    for i in idx:
        bb, be = bin_table(begin[i]), bin_table(end[i])
        if be >= BINS:
            dropped += 1
            continue
        for kind, w in ((0, w_sh[i]), (1, w_ns[i])):
            t = cells.setdefault((kind, bb, be), np.zeros(nb))
            t[block[i]] = t[block[i]] + np.float64(w)
    keys = sorted(k for k, t in cells.items() if (t > 0).any())
    g = grid()
    tables = np.array([cells[k] for k in keys]).T.reshape(nb, len(keys))
    return (np.array([k[0] for k in keys], dtype=np.int32), np.array([g[k[1]] for k in keys]), np.array([g[k[2]] for k in keys]),
            tables, dropped)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_result(got, want):
    for name, x, y in zip(("kinds", "age_begin", "age_end", "tables"), got[:4], want[:4]):
        assert same_bits(x, y), (name, x.shape, y.shape)
    assert got[4] == want[4], ("dropped", got[4], want[4])


def mixed_weights(rng, n):
    """1e-3 .. 1e3, so that another order of addition changes bits; a tenth of the shared weights zero"""
    w_sh = 10.0 ** rng.uniform(-3, 3, n) * (rng.uniform(size=n) > 0.1)
    return w_sh, 10.0 ** rng.uniform(-3, 3, n)


def random_records(n_per_block, nb, seed, empty=()):
    """ages within two decades (a few records per cell), a few from age 0, a few points, a few beyond the grid; the blocks in
    `empty` get no record"""
    rng = np.random.default_rng(seed)
    blocks = [k for k in range(nb) if k not in empty]
    n = n_per_block * len(blocks)
    begin = (10.0 ** rng.uniform(1, 3, n)).astype(np.float32)
    end = (begin * (1 + 1.5 * rng.uniform(size=n))).astype(np.float32)
    u = rng.uniform(size=n)
    begin[u < 0.08] = 0.0
    end[(u > 0.08) & (u < 0.12)] = begin[(u > 0.08) & (u < 0.12)]
    end[u > 0.98] = 3e7
    w_sh, w_ns = mixed_weights(rng, n)
    return begin, end, w_sh, w_ns, np.repeat(np.array(blocks, dtype=np.int32), n_per_block), nb


def one_cell(n, seed, bb=60, be=75, nb=1):
    rng = np.random.default_rng(seed)
    w_sh, w_ns = mixed_weights(rng, n)
    return (np.full(n, age_in_bin(bb), dtype=np.float32), np.full(n, age_in_bin(be), dtype=np.float32), w_sh, w_ns,
            np.zeros(n, dtype=np.int32), nb)


def alternating(n, seed):
    """two cells, record by record"""
    b, e, w_sh, w_ns, blk, nb = one_cell(n, seed)
    b[1::2], e[1::2] = age_in_bin(61), age_in_bin(90)
    return b, e, w_sh, w_ns, blk, nb


def tile_boundaries(seed):
    """the two cells on each side of every tile boundary of the kernel, one record each"""
    tile = colate_amd.interval_cells_tile()
    cs = [t * tile + d for t in range(1, (CELLS + tile - 1) // tile) for d in (-2, -1, 0, 1)]
    cs += [0, 1, CELLS - 2, CELLS - 1]
    cs = [c for c in cs if 0 <= c < CELLS]
    rng = np.random.default_rng(seed)
    cs = [cs[i] for i in rng.permutation(len(cs))]
    bbe = [cell_of_index(c) for c in cs]
    w_sh, w_ns = mixed_weights(rng, len(cs))
    w_sh = np.maximum(w_sh, 1e-3)
    return (np.array([age_in_bin(bb) for bb, _ in bbe], dtype=np.float32), np.array([age_in_bin(be) for _, be in bbe], dtype=np.float32),
            w_sh, w_ns, np.zeros(len(cs), dtype=np.int32), 1), cs


def special_records():
    """a record from age 0 (the reference's F path), a point record (bb == be), one of each beyond the grid"""
    begin = np.array([0.0, 500.0, 0.0, 2e4, 0.0], dtype=np.float32)
    end = np.array([800.0, 500.0, 3e7, 3e7, 0.0], dtype=np.float32)
    return begin, end, np.array([1.5, 2.0, 1.0, 1.0, 0.25]), np.array([0.5, 0.125, 1.0, 1.0, 4.0]), np.zeros(5, dtype=np.int32), 1


def cases():
    """name -> record set; the sizes are those at which the kernel takes another path: a wave's batch of 64 records and its
    edges, chains across lanes and batches, conflicts within a wave, every tile boundary, empty blocks"""
    c = {"one": one_cell(1, 1)}
    for n in (63, 64, 65):
        c[f"block_of_{n}"] = random_records(n, 1, 10 + n)
    c["one_cell_130"] = one_cell(130, 2)
    c["alternating"] = alternating(130, 3)
    c["tile_boundaries"] = tile_boundaries(4)[0]
    c["middle_block_empty"] = random_records(150, 3, 5, empty=(1,))
    c["nb1"] = random_records(300, 1, 6)
    b, e, w_sh, w_ns, blk, nb = random_records(100, 3, 7, empty=(1,))
    e[blk == 2] = 3e7  # a block with only dropped records
    c["block_all_dropped"] = (b, e, w_sh, w_ns, blk, nb)
    c["special"] = special_records()
    c["random_5x2000"] = random_records(2000, 5, 8)
    return c


# ------------------------------------------------------------------ the command line
def run_cli(args, cwd, device, timeout=120):
    env = dict(os.environ)
    env.pop("COLATE_DEVICE_INTERVAL", None)
    if not device:
        env["COLATE_DEVICE_INTERVAL"] = "0"
    return subprocess.run([CLI, "--mode", "mut_interval"] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True,
                          env=env, timeout=timeout)


def stderr_count(r, label):
    """the number after `label: ` on stderr"""
    for line in r.stderr.splitlines():
        if line.startswith(label + ": "):
            return int(line[len(label) + 2:])
    raise AssertionError((label, r.stderr[-1500:]))


def read_rows_file(path):
    """per kind the total weight of a --write_rows file, the number of distinct rows and the block ids"""
    total, rows, blocks = {"shared": 0.0, "notshared": 0.0}, set(), set()
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        b, kind, a0, a1, w = line.split()
        total[kind] += float(w)
        rows.add((kind, a0, a1))
        blocks.add(int(b))
    return total, len(rows), sorted(blocks)


def write_mask(path, n_masked):
    """a FASTA mask that removes every position below n_masked (any letter but P removes; beyond its end everything passes)"""
    with open(path, "w") as f:
        f.write(">mask\n" + "N" * n_masked + "\n")
