"""What the tests of colate_topo_profile and of `Colate --mode count_topo --age_profile` share: the contract of age_epoch
(csrc/count_topo.h) restated in numpy over the planes of the host twin of colate_topo_samples, the epochs and the edge inputs used
on both machines, and the reference's files aggregated per epoch.  The inputs, the model of the draws and the runner of the command
line are those of count_topo_lib.py, to which this adds nothing."""
import functools
import gzip
import os

import numpy as np

import colate_amd
import count_topo_lib as tl

F32 = np.float32
# E = 1, 2, 11 and 1024, every boundary a float: a mid can lie on one exactly.  The ages of the edge cases have mids of about
# 15 to 2500 generations (interval_walk_lib.make_rows), which 0 .. 256 and 0 .. 2557.5 spread over the epochs.
EPOCHS = {1: np.array([0.0]), 2: np.array([0.0, 64.0]), 11: np.array([0.0, 0.5] + [2.0 ** k for k in range(9)]), 1024: np.arange(1024) * 2.5}
ONE_EPOCH_OF_TWO = np.array([0.0, 1e9])  # every row of every chromosome in epoch 0 of 2: 64 lanes of a word add to one address
BINS = "3,7,0.5"                         # the command line's spec on the fixture: 11 epochs at 28 years per generation


def above(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def age_epoch(begin, end, epochs):
    """the contract: the mid formed in float32 -- one addition, rounded, and an exact halving --, the number of e in 1 .. E - 1
    with epochs[e] <= mid; a NaN mid gives 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        mid = F32(0.5) * (np.asarray(begin, dtype=F32) + np.asarray(end, dtype=F32))
    assert mid.dtype == F32
    e = np.searchsorted(np.asarray(epochs, dtype=np.float64)[1:], mid.astype(np.float64), "right")
    return np.where(np.isnan(mid), 0, e).astype(np.int64)


def unpack(plane, row_off):
    """the inverse of count_topo_lib.pack: one 0 / 1 per row from the words of one triple's plane"""
    out, w = [], 0
    for c in range(len(row_off) - 1):
        n = int(row_off[c + 1] - row_off[c])
        words = (n + 63) // 64
        out.append(np.unpackbits(plane[w:w + words].view(np.uint8), bitorder="little")[:n])
        w += words
    return np.concatenate(out).astype(bool) if out else np.zeros(0, dtype=bool)


def model(c, epochs, planes=None):
    """(counts [P, E, 3], draws [P]) of a case: the planes of the host twin of colate_topo_samples (or those given), Q by the rule
    of count_topo_lib.model, the rows' epochs by age_epoch above"""
    _, plus, minus, draws = tl.topo(c, device=False) if planes is None else planes
    hit = (c["idx"]["DAF"] | c["idx"]["AAF"]) != 0
    qual = c["cond_idx"]["DAF"] > 0
    E = len(epochs)
    e = age_epoch(c["rows"]["age_begin"], c["rows"]["age_end"], epochs)
    counts = np.zeros((len(c["triples"]), E, 3), dtype=np.int64)
    for p, t in enumerate(c["triples"]):
        q = hit[int(t["target"])] & hit[int(t["reference"])] & qual[int(t["cond"])]
        assert int(q.sum()) == int(draws[p])
        for k, bits in enumerate((unpack(plus[p], c["row_off"]), unpack(minus[p], c["row_off"]), q)):
            counts[p, :, k] = np.bincount(e[bits], minlength=E)
    return counts, np.asarray(draws, dtype=np.int64)


def profile(c, epochs, device):
    return colate_amd.topo_profile(c["row_off"], c["rows"], c["idx"], c["cond_idx"], c["triples"], c["uniforms"], epochs, device=device)


def assert_same(got, want):
    for name, x, y in zip(("counts", "draws"), got, want):
        assert x.dtype == np.int64 and x.shape == y.shape and (x == y).all(), (name, x.shape, y.shape, np.argwhere(x != y)[:8])


def assert_invariants(c, out, planes):
    counts, draws = out
    _, plus, minus, _ = planes
    popc = lambda a: np.array([sum(bin(int(w)).count("1") for w in row) for row in a], dtype=np.int64)  # noqa: E731
    assert (counts[:, :, 2].sum(axis=1) == draws).all()
    assert (counts[:, :, 0].sum(axis=1) == popc(plus)).all() and (counts[:, :, 1].sum(axis=1) == popc(minus)).all()
    assert (counts[:, :, 0] + counts[:, :, 1] <= counts[:, :, 2]).all() and (counts >= 0).all()


@functools.lru_cache(maxsize=None)
def cases():
    """the edge cases of count_topo_lib -- chromosomes of 0, 1, 63, 64, 65 and 200 rows; TILE - 1, TILE and TILE + 1 -- and one of
    5 TILE + 3 rows behind a short one: every wave of a draw workgroup owns a tile, one owns two, and the last tile is partial"""
    return dict(tl.cases(), long=tl.edge_case([3, 5 * tl.TILE + 3], 43))


@functools.lru_cache(maxsize=None)
def twin_planes(name):
    return tl.topo(cases()[name], device=False)


@functools.lru_cache(maxsize=None)
def modelled(name, E):
    return model(cases()[name], EPOCHS[E], twin_planes(name))


# ------------------------------------------------------------------ rows on the edges of the epochs
@functools.lru_cache(maxsize=None)
def edge_rows(E):
    """One chromosome whose every row qualifies for every triple, so `qualifying` counts the rows of an epoch, with ages on, one
    float below and one float above boundaries of EPOCHS[E] -- as age_begin == age_end rows and as intervals whose float sum is
    exact --, below epochs[1], negative, above the last epoch, infinite and NaN.  Three samples in four permutations of the roles.
    Returns (case, the epoch of every row)."""
    epochs = EPOCHS[E]
    rng = np.random.default_rng(70 + E)
    ages, want = [], []
    for k in sorted({1, 2, E // 2, E - 1} & set(range(1, E))):
        b = F32(epochs[k])
        assert float(b) == epochs[k] and b > 0
        lo, hi = F32(tl.down(b)), above(b)
        assert lo < b < hi
        ages += [(b, b), (lo, lo), (hi, hi), (F32(0.5) * b, F32(1.5) * b), (lo, b), (b, hi)]
        # (lo + b and b + hi are ties of the float addition or exact: what the hardware's rounding gives is the model's, below)
        want += [k, k - 1, k, k, None, None]
    ages += [(F32(0.0), F32(0.0)), (F32(-9.0), F32(-2.0)), (F32(-3.0), F32(3.0)), (F32(np.nan), F32(5.0)), (F32(7.0), F32(np.nan)),
             (F32(1e30), F32(np.inf)), (F32(3e38), F32(3e38)), (F32(epochs[-1]) * F32(4) + F32(1), F32(epochs[-1]) * F32(4) + F32(1))]
    below1 = 0 if E == 1 or epochs[1] > 0 else 1
    want += [below1, 0, below1, 0, 0, E - 1, E - 1, E - 1]  # (3e38 + 3e38 overflows to +inf: E - 1)
    n = len(ages)
    rows = np.zeros(n, dtype=colate_amd.WALK_ROW)
    rows["pos"] = 10 + 3 * np.arange(n)
    rows["age_begin"], rows["age_end"] = [a for a, _ in ages], [b for _, b in ages]
    modelled_epoch = age_epoch(rows["age_begin"], rows["age_end"], epochs)
    for i, w in enumerate(want):
        assert w is None or modelled_epoch[i] == w, (E, i, ages[i], w, modelled_epoch[i])
    idx = np.zeros((3, n), dtype=colate_amd.WALK_IDX)
    idx["DAF"], idx["AAF"] = rng.integers(0, 4, (3, n)), rng.integers(1, 4, (3, n))
    cidx = idx.copy()
    cidx["DAF"] = rng.integers(1, 5, (3, n))
    triples = np.array([(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)], dtype=colate_amd.TOPO_TRIPLE)
    c = dict(row_off=np.array([0, n], dtype=np.int64), rows=rows, idx=idx, cond_idx=cidx, triples=triples, uniforms=rng.uniform(size=2 * n))
    return c, modelled_epoch


def assert_edge_rows(E, out):
    c, epoch = edge_rows(E)
    counts, draws = out
    assert (draws == c["rows"].size).all()
    for p in range(len(c["triples"])):
        assert (counts[p, :, 2] == np.bincount(epoch, minlength=E)).all(), (E, p)
    assert_same(out, model(c, EPOCHS[E]))


# ------------------------------------------------------------------ the fixture: the reference's files per epoch
def searched_rows(d, chroms):
    """{chromosome: (pos, age_begin, age_end as float32)} of the rows `--mode count_topo` searches, from the staged .mut files"""
    out = {}
    for ch in chroms:
        path = os.path.join(str(d), f"P_chr{ch}.mut")
        f = gzip.open(path + ".gz", "rt") if os.path.exists(path + ".gz") else open(path)
        pos, begin, end = [], [], []
        for line in f.read().splitlines()[1:]:
            x = line.split(";")
            b, e = F32(x[8]), F32(x[9])
            alleles = x[10].split("/")
            if int(x[7]) == 0 and len(x[5].split()) == 1 and b <= e and len(alleles) == 2 and all(len(a) == 1 and a in "ACGT01" for a in alleles):
                pos.append(int(x[1])), begin.append(b), end.append(e)
        f.close()
        out[ch] = (np.array(pos), np.array(begin, dtype=F32), np.array(end, dtype=F32))
    return out


def reference_profile(d, meta, epochs):
    """counts [P, E, 2] -- plus and minus -- of the reference's expected_*.txt files: every line matched to its searched row by
    chromosome, position and printed ages and binned with the row's own floats.  The match is asserted to be unique in those
    floats: the .mut files of the fixture hold a few rows twice, verbatim, and the copies of a row cannot differ in their epoch."""
    chroms = open(os.path.join(str(d), "chr.txt")).read().split()
    rows = searched_rows(d, chroms)
    printed = {ch: np.array(["%g %g" % (float(b), float(e)) for b, e in zip(r[1], r[2])]) for ch, r in rows.items()}
    counts = np.zeros((len(meta["triples"]), len(epochs), 2), dtype=np.int64)
    for p, t in enumerate(meta["triples"]):
        for line in open(os.path.join(str(d), t["output"])).read().splitlines():
            x = line.split(" ")
            pos, _, _ = rows[x[0]]
            at = np.nonzero((pos == int(x[1])) & (printed[x[0]] == x[2] + " " + x[3]))[0]
            # unique in what decides the epoch: the fixture repeats some .mut rows verbatim, and such copies carry the same floats
            floats = {(rows[x[0]][1][i].tobytes(), rows[x[0]][2][i].tobytes()) for i in at}
            assert len(floats) == 1, (t["output"], line, at)
            i = int(at[0])
            e = int(age_epoch(rows[x[0]][1][i:i + 1], rows[x[0]][2][i:i + 1], epochs)[0])
            counts[p, e, 0 if int(x[4]) > 0 else 1] += 1
    return counts


def read_profile(path, meta, E):
    """PREFIX.profile.txt as (names per triple, the printed epochs, counts [P, E, 3]); the layout is asserted"""
    lines = open(str(path)).read().splitlines()
    P = len(meta["triples"])
    assert len(lines) == P * E
    counts = np.zeros((P, E, 3), dtype=np.int64)
    printed = []
    for k, line in enumerate(lines):
        x = line.split(" ")
        assert len(x) == 7 and x[:3] == meta["triples"][k // E]["names"], line
        counts[k // E, k % E] = [int(v) for v in x[4:]]
        if k < E:
            printed.append(x[3])
        else:
            assert x[3] == printed[k % E]
    return printed, counts
