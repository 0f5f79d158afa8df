"""What the tests of colate_topo_samples and of `Colate --mode count_topo` share: the contract of csrc/count_topo.h restated as a
numpy model (independent of the C++), the edge inputs used on both machines -- built with the helpers of interval_walk_lib.py --,
small inputs as FILES for the cursor walk, and the fixture's staging and CLI runner."""
import functools
import gzip
import json
import os
import shutil
import struct
import subprocess

import numpy as np

import colate_amd
import interval_cells_lib as il
import interval_walk_lib as wl

FIXTURE = os.path.join(il.HERE, "golden", "count_topo")
TILE = colate_amd.topo_samples_tile()
# the samples of an edge case
RANDOM0, RANDOM1, RANDOM2, FULL, EMPTY, FULL2, SPARSE = range(7)
TRIPLES = [(RANDOM0, RANDOM1, RANDOM2),  # (cond, target, reference)
           (RANDOM1, RANDOM2, RANDOM0),  # sample 2 is the reference above and the target here
           (FULL, FULL, FULL),           # every row qualifies: rank = row
           (RANDOM0, EMPTY, RANDOM1),    # the target never hits: no qualifying row
           (EMPTY, RANDOM0, RANDOM1),    # a cond index that qualifies where the walk index of the same sample does not hit
           (FULL, FULL, FULL2),          # every row qualifies, target and reference differ: the injected uniforms decide
           (FULL, SPARSE, FULL),         # Q only in the last bit of one word and in the first bit of another
           (RANDOM2, FULL2, RANDOM1)]
ALL_ROWS, NO_ROW, COND_ONLY, INJECTED, SPARSE_Q = 2, 3, 4, 5, 6  # triples by what they are for


# ------------------------------------------------------------------ the contract, as numpy
def pack(bits, row_off):
    """one array of 0 / 1 over all rows as plane words, each chromosome starting on a word"""
    out = []
    for c in range(len(row_off) - 1):
        b = np.asarray(bits[int(row_off[c]):int(row_off[c + 1])], dtype=np.uint8)
        b = np.concatenate([b, np.zeros(-b.size % 64, dtype=np.uint8)])
        out.append(np.packbits(b, bitorder="little").view(np.uint64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


def model(c):
    """(word_off, plus [P][words], minus [P][words], draws [P]) of a case; raises where the stream is too short"""
    row_off, idx, cidx, u = c["row_off"], c["idx"], c["cond_idx"], np.asarray(c["uniforms"], dtype=np.float64)
    word_off = np.concatenate([[0], np.cumsum((np.diff(row_off) + 63) // 64)]).astype(np.int64)
    hit = (idx["DAF"] | idx["AAF"]) != 0
    qual = cidx["DAF"] > 0
    N = idx["DAF"].astype(np.int64) + idx["AAF"]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = idx["DAF"].astype(np.float64) / N
    plus, minus, draws = [], [], []
    for t in c["triples"]:
        q = hit[int(t["target"])] & hit[int(t["reference"])] & qual[int(t["cond"])]
        rank = np.cumsum(q) - 1  # the rows are back to back, chromosome after chromosome: the rank runs on
        n = int(q.sum())
        if 2 * n > u.size:
            raise ValueError(f"needed: {2 * n}")
        at = rank[q]
        d1, d2 = u[2 * at].astype(np.float32).astype(np.float64), u[2 * at + 1].astype(np.float32).astype(np.float64)
        pT, pR = p[int(t["target"])][q], p[int(t["reference"])][q]
        a, b = np.zeros(q.size, dtype=np.uint8), np.zeros(q.size, dtype=np.uint8)
        a[q] = (d1 <= pT) & (d2 > pR)
        b[q] = (d1 > pT) & (d2 <= pR)
        plus.append(pack(a, row_off)), minus.append(pack(b, row_off)), draws.append(n)
    return word_off, np.array(plus, dtype=np.uint64).reshape(len(draws), -1), np.array(minus, dtype=np.uint64).reshape(len(draws), -1), \
        np.array(draws, dtype=np.int64)


def topo(c, device, cap=None):
    return colate_amd.topo_samples(c["row_off"], c["rows"], c["idx"], c["cond_idx"], c["triples"], c["uniforms"], device=device, cap=cap)


NAMES = ("word_off", "plus", "minus", "draws")


def assert_same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert il.same_bits(x, y), (name, x.shape, y.shape, np.argwhere(x != y)[:8] if x.shape == y.shape else None)


def bit(plane, c, p, g):
    """bit of global row g in triple p's plane"""
    row_off = c["row_off"]
    ch = int(np.searchsorted(row_off, g, side="right")) - 1
    word_off = np.concatenate([[0], np.cumsum((np.diff(row_off) + 63) // 64)])
    i = g - int(row_off[ch])
    return (int(plane[p, word_off[ch] + (i >> 6)]) >> (i & 63)) & 1


# ------------------------------------------------------------------ the edge inputs
F32 = np.float32


def up(x):
    return float(np.nextafter(F32(x), F32(2)))


def down(x):
    return float(np.nextafter(F32(x), F32(-1)))


# (target counts (DAF, AAF), reference counts, u1, u2, the sign) at consecutive rows of the INJECTED triple
INJECT = [((1, 3), (1, 3), 0.25, up(0.25), 1),                      # (float)u1 == pT exactly: `<=` holds; d2 one float above pR
          ((1, 3), (1, 3), up(0.25), 0.25, -1),                     # one float above pT; (float)u2 == pR exactly
          ((1, 3), (1, 3), 0.25, 0.25, 0),                          # both on the quotient: d2 > pR fails, d1 > pT fails
          ((1, 3), (1, 3), down(0.25), up(0.25), 1),                # one float below, one above
          ((1, 3), (1, 3), 0.25 + 2.0 ** -40, 0.25 - 2.0 ** -40, 0),  # doubles off the quotient that round to it as floats
          ((1, 3), (1, 3), 0.25 + 2.0 ** -40, up(0.25), 1),         # ... above as a double, on it as a float
          ((2, 0), (0, 2), 1.0 - 2.0 ** -53, 2.0 ** -60, 1),          # u1 rounds to 1.0f against pT == 1; d2 > 0 == pR
          ((2, 0), (2, 0), 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53, 0),    # 1.0f <= 1 on both sides
          ((0, 2), (0, 2), 0.0, 0.0, 0),                              # u == 0 against p == 0: `<=` on both sides
          ((0, 2), (0, 2), 2.0 ** -60, 0.0, -1),                      # d1 > 0 == pT, u2 == 0 <= pR == 0
          ((0, 2), (1, 1), 0.0, 0.75, 1),                             # u1 == 0 <= pT == 0
          ((1, 2), (2, 1), float(F32(1.0) / F32(3.0)), 0.9, 0)]       # 1 / 3 as a float lies above 1 / 3 as a double


def edge_case(ns, seed):
    """Seven samples over chromosomes of ns rows (the last one at least 200): three random ones; FULL and FULL2, which hit and
    qualify everywhere; EMPTY, whose walk index never hits and whose cond index always qualifies; SPARSE, which hits a last and
    a first bit of a word only.  The stream is exactly as long as the longest triple needs: two uniforms per row."""
    rng = np.random.default_rng(seed)
    row_off, rows = wl.make_rows(ns, rng, 3)
    n = rows.size
    idx = wl.make_idx(7, row_off, rows, rng)
    cidx = wl.make_idx(7, row_off, rows, rng, zero=0.4)
    for s in (FULL, FULL2):
        idx["DAF"][s], idx["AAF"][s] = rng.integers(0, 4, n), rng.integers(1, 4, n)
        cidx["DAF"][s] = rng.integers(1, 5, n)
    idx["DAF"][EMPTY], idx["AAF"][EMPTY], cidx["DAF"][EMPTY] = 0, 0, rng.integers(1, 3, n)
    last = int(row_off[-2])
    assert n - last >= 200
    idx["DAF"][SPARSE], idx["AAF"][SPARSE] = 0, 0
    idx["DAF"][SPARSE, last + 127], idx["AAF"][SPARSE, last + 192] = 2, 1  # bit 63 of word 1, bit 0 of word 3
    u = rng.uniform(size=2 * n)
    g0 = last + 122  # the injected rows: across the edge of words 1 and 2 of the last chromosome
    for k, (t, r, u1, u2, _) in enumerate(INJECT):
        idx["DAF"][FULL, g0 + k], idx["AAF"][FULL, g0 + k] = t
        idx["DAF"][FULL2, g0 + k], idx["AAF"][FULL2, g0 + k] = r
        u[2 * (g0 + k)], u[2 * (g0 + k) + 1] = u1, u2
    triples = np.array(TRIPLES, dtype=colate_amd.TOPO_TRIPLE)
    return dict(row_off=row_off, rows=rows, idx=idx, cond_idx=cidx, triples=triples, uniforms=u, injected_at=g0)


@functools.lru_cache(maxsize=None)
def cases():
    """sizes: chromosomes of 0, 1, 63, 64 and 65 searched rows (and one of 200 for the crafted rows) in one call.  tiles: one row
    below, exactly and one row above the tile of the draw kernel: the ranks run on across chromosome and tile boundaries."""
    return {"sizes": edge_case([0, 1, 63, 64, 65, 200], 41), "tiles": edge_case([TILE - 1, TILE, TILE + 1], 42)}


@functools.lru_cache(maxsize=None)
def modelled(name):
    return model(cases()[name])


def assert_edges(name, out):
    """the case is what it says, in the outputs given"""
    c = cases()[name]
    n = c["rows"].size
    _, plus, minus, draws = out
    assert draws[ALL_ROWS] == n and draws[INJECTED] == n and draws[NO_ROW] == 0 and draws[SPARSE_Q] == 2
    assert 2 * n == c["uniforms"].size  # the stream is exactly as long as needed
    assert not plus[NO_ROW].any() and not minus[NO_ROW].any()
    assert 0 < draws[COND_ONLY] and 0 < draws[0] < n and (plus & minus == 0).all()
    for k, (_, _, _, _, sign) in enumerate(INJECT):
        g = c["injected_at"] + k
        assert (bit(plus, c, INJECTED, g), bit(minus, c, INJECTED, g)) == (int(sign > 0), int(sign < 0)), (k, INJECT[k])
    for p in (0, 1, INJECTED, len(TRIPLES) - 1):
        assert plus[p].any() and minus[p].any(), p


# ------------------------------------------------------------------ small inputs as files, for the cursor walk
def write_file_case(d, seed=51, chroms=("1", "2"), n=300, big_counts=False):
    """P_chr<c>.mut and s0 .. s3.colate.in under d: rows at equal positions, rows only this mode searches (age_begin == age_end,
    age_end < 0), rows it does not, records between the rows, samples that end before a chromosome's last rows (the conditioning
    record is then the next chromosome's first, or the file's last).  Returns the case as topo_samples takes it, walk and cond
    indices formed here by the rule of the header, without the stream.  big_counts: sample 2 with counts beyond 16 bits."""
    rng = np.random.default_rng(seed)
    bases = "ACGT"
    S = 4
    files = [open(os.path.join(d, f"s{s}.colate.in"), "wb") for s in range(S)]
    all_recs = [[] for _ in range(S)]  # (chrom index, bp, anc, der, aaf, daf) in file order
    searched_all, row_off = [], [0]
    for ci, ch in enumerate(chroms):
        pos = np.sort(rng.integers(1000, 100000, n))
        pos[5:12] = pos[5]
        pos = np.sort(pos)
        recs = [[] for _ in range(S)]
        searched = []
        stop = [pos[-1] + 1, pos[-20], pos[-1] + 1, pos[-40]]  # samples 1 and 3 end before the chromosome's last rows
        with open(os.path.join(d, f"P_chr{ch}.mut"), "w") as f:
            f.write("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                    "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n")
            for i, bp in enumerate(pos):
                a = bases[rng.integers(4)]
                der = bases[(bases.index(a) + rng.integers(1, 4)) % 4]
                u = rng.uniform()
                begin, end = (-9.0, -2.0) if u < 0.1 else (100.0, 100.0) if u < 0.2 else (900.0, 50.0) if u < 0.25 else (50.0, 900.0)
                flipped, branches = int(rng.uniform() < 0.05), "7" if rng.uniform() > 0.05 else "7 12"
                f.write(f"{i};{bp};1;rs{i};{i // 10};{branches};0;{flipped};{begin:.6g};{end:.6g};{a}/{der};{a};{der};\n")
                if flipped == 0 and branches == "7" and begin <= end:
                    searched.append((int(bp), a, der, begin, end))
                for s in range(S):
                    if bp >= stop[s]:
                        continue
                    if rng.uniform() < 0.8:
                        cnt = int(rng.integers(0, 5)) * (30000 if big_counts and s == 2 else 1)
                        daf = int(rng.integers(0, cnt + 1))
                        ra, rd = (a, der) if rng.uniform() > 0.05 else (der, a)
                        recs[s].append((ci, int(bp), ra, rd, cnt - daf, daf))
                    if rng.uniform() < 0.1:
                        recs[s].append((ci, int(bp) + 1, "A", "G", 1, 1))
        for s in range(S):
            recs[s].sort(key=lambda r: r[1])
            all_recs[s] += recs[s]
        searched_all.append(searched)
        row_off.append(row_off[-1] + len(searched))
    for s in range(S):
        for ci, bp, ra, rd, aaf, daf in all_recs[s]:
            c = chroms[ci].encode()
            files[s].write(struct.pack("<i", len(c)) + c + struct.pack("<i", bp) + ra.encode() + rd.encode() + struct.pack("<ii", aaf, daf))
        files[s].close()
    with open(os.path.join(d, "chr.txt"), "w") as f:
        f.write("".join(c + "\n" for c in chroms))
    with open(os.path.join(d, "samples.txt"), "w") as f:
        f.write("".join(f"s{s} s{s}.colate.in\n" for s in range(S)))
    if big_counts:  # (counts beyond the 16 bits of an index: the files only)
        return None
    idx, cidx = np.zeros((S, row_off[-1]), dtype=wl.IDX), np.zeros((S, row_off[-1]), dtype=wl.IDX)
    for s in range(S):
        R = all_recs[s]
        for ci in range(len(chroms)):
            run = [k for k, r in enumerate(R) if r[0] == ci]
            b, e = run[0], run[-1] + 1
            bps = np.array([R[k][1] for k in range(b, e)], dtype=np.int64)
            for i, (bp, a, der, _, _) in enumerate(searched_all[ci]):
                k = b + int(np.searchsorted(bps, bp, side="left"))  # the lower bound; e: behind the chromosome's last record
                g = row_off[ci] + i
                if k < e and R[k][1] == bp and R[k][2] == a and R[k][3] == der:
                    idx["DAF"][s, g], idx["AAF"][s, g] = R[k][5], R[k][4]
                idx["prev_bp"][s, g] = R[k - 1][1] if b < k < e else -2
                at = R[k] if k < e else R[e] if e < len(R) else R[-1]
                cidx["DAF"][s, g], cidx["AAF"][s, g] = at[5], at[4]
    rows = np.zeros(row_off[-1], dtype=wl.ROW)
    flat = [x for sr in searched_all for x in sr]
    rows["pos"], rows["age_begin"], rows["age_end"] = [x[0] for x in flat], [x[3] for x in flat], [x[4] for x in flat]
    triples = np.array([(c, t, r) for c in range(S) for t in range(S) for r in range(S) if len({c, t, r}) == 3], dtype=colate_amd.TOPO_TRIPLE)
    return dict(row_off=np.array(row_off, dtype=np.int64), rows=rows, idx=idx, cond_idx=cidx, triples=triples, chroms=chroms)


def mt_uniforms(seed, n):
    """the first n values of uniform_real_distribution<double>(0, 1) over std::mt19937(seed): two 32-bit words each, the low one
    first, over 2^64 (numpy's MT19937 seeded the same way gives the same words)"""
    legacy = np.random.RandomState(seed).get_state()  # init_genrand(seed): std::mt19937's seeding
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": legacy[1], "pos": legacy[2]}}
    words = bg.random_raw(2 * n).astype(np.uint64)
    x = (words[0::2].astype(np.longdouble) + words[1::2].astype(np.longdouble) * np.longdouble(2.0 ** 32)) / np.longdouble(2.0 ** 64)
    x = x.astype(np.float64)
    return np.where(x >= 1.0, np.nextafter(1.0, 0.0), x)


def lines_of(c, out, p):
    """the file of triple p from the planes: `name pos age_begin age_end sign value` as (name, pos, sign, DAF_cond, N_cond)"""
    _, plus, minus, _ = out
    got = []
    t = c["triples"][p]
    for g in range(c["rows"].size):
        a, b = bit(plus, c, p, g), bit(minus, c, p, g)
        if a or b:
            ch = int(np.searchsorted(c["row_off"], g, side="right")) - 1
            x = c["cond_idx"][int(t["cond"])][g]
            got.append((c["chroms"][ch], int(c["rows"]["pos"][g]), 1 if a else -1, int(x["DAF"]), int(x["DAF"]) + int(x["AAF"])))
    return got


def read_lines(path):
    out = []
    for line in open(path).read().splitlines():
        x = line.split(" ")
        out.append((x[0], int(x[1]), int(x[4]), float(x[5])))
    return out


# ------------------------------------------------------------------ the fixture and the command line
def stage(d, sub=""):
    """the fixture (or its nochr/ part) under d with the .colate.in files inflated; returns case.json"""
    src = os.path.join(FIXTURE, sub)
    for fn in os.listdir(src):
        if fn.endswith(".colate.in.gz"):
            with gzip.open(os.path.join(src, fn), "rb") as g, open(os.path.join(d, fn[:-3]), "wb") as f:
                f.write(g.read())
        elif os.path.isfile(os.path.join(src, fn)):
            shutil.copy(os.path.join(src, fn), os.path.join(d, fn))
    return json.load(open(os.path.join(src, "case.json")))


ENV_KEYS = ("COLATE_DEVICE_TOPO", "COLATE_INDEXED_WALK", "COLATE_TOPO_BUDGET")


def run_cli(d, args, env=None, timeout=120):
    """`Colate --mode count_topo ARGS` in d; env: COLATE_DEVICE_TOPO and the like (those of the caller's are dropped)"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([il.CLI, "--mode", "count_topo"] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, env=e,
                          timeout=timeout)


HOST = {"COLATE_DEVICE_TOPO": "0"}
CURSORS = {"COLATE_DEVICE_TOPO": "0", "COLATE_INDEXED_WALK": "0"}


def assert_samples_files(d, meta, prefix):
    """every triple's file is the reference's, and PREFIX.triples.txt holds the totals in triple order"""
    lines = (d / f"{prefix}.triples.txt").read_text().splitlines()
    assert len(lines) == len(meta["triples"])
    for line, p in zip(lines, meta["triples"]):
        c, t, r = p["names"]
        mine, want = (d / f"{prefix}_{c}_{t}_{r}.txt").read_bytes(), (d / p["output"]).read_bytes()
        assert len(want) > 100 and mine == want, (c, t, r)
        x = line.split(" ")
        assert x[:5] == [c, t, r, str(p["plus"]), str(p["minus"])] and int(x[5]) >= p["plus"] + p["minus"], (line, p["names"])
