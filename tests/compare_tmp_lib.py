"""What the tests of colate_compare_samples and of `Colate --mode compare_tmp` share: the contract of csrc/compare_tmp.h
restated as a stateless numpy model (independent of the C++), the edge inputs used on both machines -- built with the helpers
of interval_walk_lib.py --, small inputs as FILES for the cursor walk, and the fixture's staging and CLI runner."""
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

FIXTURE = os.path.join(il.HERE, "golden", "compare_tmp")
BINSIZE = 10_000_000
ALL_PAIRS = [(a, b) for a in range(3) for b in range(3) if a != b]  # S = 3: all six ordered pairs


# ------------------------------------------------------------------ the contract, as numpy
def window_of(pos, first, window):
    pos = np.asarray(pos, dtype=np.int64)
    return np.where(pos > first, (pos - first - 1) // window, 0)


def model(c):
    """(win_off, mismatch [P][W], snps [P][W]) of a case: hit and fixed per sample and row, bincounts per pair"""
    row_off, rows, idx, pairs = c["row_off"], c["rows"], c["idx"], c["pairs"]
    C = len(row_off) - 1
    win_off, mm, n = [0], [[] for _ in pairs], [[] for _ in pairs]
    for ch in range(C):
        lo, hi = int(row_off[ch]), int(row_off[ch + 1])
        pos = rows["pos"][lo:hi].astype(np.int64)
        prev = np.concatenate([[-1], pos[:-1]])[:pos.size]  # pos(-1) = -1 at the chromosome's start
        x = idx[:, lo:hi]
        hit = ((x["DAF"] | x["AAF"]) != 0) & (x["prev_bp"].astype(np.int64) >= prev)
        fixed = x["AAF"] == 0
        first, last = int(c["first_pos"][ch]), int(c["last_pos"][ch])
        W = int(window_of(last, first, c["window"])) + 1
        w = window_of(pos, first, c["window"])
        for p, pr in enumerate(pairs):
            t, r = int(pr["target"]), int(pr["reference"])
            both = hit[t] & hit[r]
            n[p].append(np.bincount(w[both], minlength=W))
            mm[p].append(np.bincount(w[both & (fixed[t] != fixed[r])], minlength=W))
        win_off.append(win_off[-1] + W)
    cat = lambda per_pair: np.array([np.concatenate(x) for x in per_pair], dtype=np.int32).reshape(len(pairs), win_off[-1])  # noqa: E731
    return np.array(win_off, dtype=np.int64), cat(mm), cat(n)


def compare(c, device, cap=None):
    return colate_amd.compare_samples(c["row_off"], c["rows"], c["idx"], c["pairs"], c["first_pos"], c["last_pos"], c["window"],
                                      device=device, cap=cap)


NAMES = ("win_off", "mismatch", "snps")


def assert_same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert il.same_bits(x, y), (name, x.shape, y.shape, np.argwhere(x != y)[:8] if x.shape == y.shape else None)


def assert_symmetric(c, out):
    """(a, b) and (b, a) alike; mismatch <= snps everywhere"""
    _, mm, n = out
    assert (mm <= n).all() and (mm >= 0).all()
    at = {(int(p["target"]), int(p["reference"])): j for j, p in enumerate(c["pairs"])}
    for (t, r), j in at.items():
        if (r, t) in at:
            assert (mm[j] == mm[at[(r, t)]]).all() and (n[j] == n[at[(r, t)]]).all(), (t, r)


# ------------------------------------------------------------------ the edge inputs
def make_case(ns, seed, window, step=3, lead=3, tail_windows=5, jumps=0.04):
    """chromosomes of ns rows, positions about one base apart with equal positions and some jumps of several windows (empty
    windows); first_pos `lead` bases below the first row, last_pos some windows beyond the last one"""
    rng = np.random.default_rng(seed)
    row_off, rows = wl.make_rows(ns, rng, step)
    for ch in range(len(ns)):  # jumps: windows without any row
        lo, hi = int(row_off[ch]), int(row_off[ch + 1])
        j = (rng.uniform(size=hi - lo) < jumps) * rng.integers(2 * window, 6 * window, hi - lo)
        rows["pos"][lo:hi] += np.cumsum(j).astype(np.int32)
    idx = wl.make_idx(3, row_off, rows, rng)
    first = np.array([int(rows["pos"][row_off[ch]]) - lead if ns[ch] else 100 for ch in range(len(ns))], dtype=np.int32)
    last = np.array([int(rows["pos"][row_off[ch + 1] - 1]) + tail_windows * window + 3 if ns[ch] else 100 + 4 * window + 1
                     for ch in range(len(ns))], dtype=np.int32)
    return dict(row_off=row_off, rows=rows, idx=idx, pairs=wl.make_pairs(ALL_PAIRS), first_pos=first, last_pos=last, window=window)


def sizes_case():
    """1, 63, 64, 65, 256 and 257 searched rows and a chromosome without any, in one call: planes cross word and tile
    boundaries, every chromosome starts on a word.  window = 7 over positions 0 .. 2 apart: a 64-row word holds three window
    boundaries and more; the dense positions lie on first + 7 k and on first + 7 k + 1; jumps leave windows empty."""
    c = make_case([1, 63, 64, 65, 0, 256, 257], 21, 7)
    rows, row_off, idx = c["rows"], c["row_off"], c["idx"]
    lo = int(row_off[5])
    rows["pos"][lo:lo + 40] = c["first_pos"][5] + 7 * 2 + np.repeat(np.arange(20), 2)  # pairs of equal positions over the window edges
    rows["pos"][lo + 40:int(row_off[6])] = np.maximum(rows["pos"][lo + 40:int(row_off[6])], rows["pos"][lo + 39])
    rows["pos"][lo:int(row_off[6])] = np.maximum.accumulate(rows["pos"][lo:int(row_off[6])])
    c["last_pos"][5] = rows["pos"][int(row_off[6]) - 1] + 40
    for s in range(3):
        x = idx[s]
        for i in range(lo, lo + 40):  # as a file's index has it: the first of two equal rows can hit, the second cannot
            x[i] = (rows["pos"][i] - 1, 1 + (i + s) % 3, (i * (s + 1)) % 2)
        x[lo] = (-2, 2, 1)  # the lower bound is the chromosome's first record: no hit at the first row
        x[lo + 41] = (-2, 1, 1)
        x[lo + 50] = (rows["pos"][lo + 49], 0, 0)  # a record without counts
        # the first row of chromosome 2 (63 rows): chromosome 1's only row lies far above it
        x[int(row_off[1])] = (0, 1, s % 2)
    rows["pos"][0] = 5000
    c["first_pos"][0], c["last_pos"][0] = 4990, 5000
    assert (np.diff(rows["pos"][lo:int(row_off[6])]) >= 0).all() and rows["pos"][int(row_off[1])] < 5000
    return c


def many_windows_case():
    """window = 1 over 3000 rows: a few thousand windows, every wave of a workgroup takes hundreds"""
    return make_case([3000, 70], 22, 1, step=4, jumps=0.0)


def wide_window_case():
    """one window holds the whole chromosome of several hundred words: the lanes stride"""
    return make_case([64 * 70 + 9, 5], 23, 1_000_000, jumps=0.0)


@functools.lru_cache(maxsize=None)
def cases():
    return {"sizes": sizes_case(), "many_windows": many_windows_case(), "wide_window": wide_window_case()}


@functools.lru_cache(maxsize=None)
def modelled(name):
    return model(cases()[name])


# ------------------------------------------------------------------ small inputs as files, for the cursor walk
def write_file_case(d, seed=31, chroms=("1", "2"), n=260):
    """P_chr<c>.mut and s0 .. s2.colate.in under d, positions on first + k 10 Mb and one above among them, a window without rows, rows at equal
    positions, rows only this mode searches (age_end < 0), rows it does not; returns the case as compare_samples takes it
    (the index of every sample formed here, by the rule of build_walk_index)"""
    rng = np.random.default_rng(seed)
    bases = "ACGT"
    files = [open(os.path.join(d, f"s{s}.colate.in"), "wb") for s in range(3)]
    rows, idx, row_off, first_pos, last_pos = [], [[], [], []], [0], [], []
    for ch in chroms:
        first = int(rng.integers(1000, 50000))
        pos = np.sort(np.concatenate([[first], first + BINSIZE * rng.integers(1, 5, n // 8), first + 1 + BINSIZE * rng.integers(1, 5, n // 8),
                                      first + rng.integers(1, 5 * BINSIZE, n - 2 * (n // 8) - 2), [first + 6 * BINSIZE + 17]]))  # (window 5 is empty)
        pos[5:25] = pos[5]  # a run of equal positions
        pos = np.sort(pos)
        recs = [[] for _ in range(3)]
        searched = []
        with open(os.path.join(d, f"P_chr{ch}.mut"), "w") as f:
            f.write("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                    "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n")
            for i, bp in enumerate(pos):
                a = bases[rng.integers(4)]
                der = bases[(bases.index(a) + rng.integers(1, 4)) % 4]
                u = rng.uniform()
                begin, end = (-9.0, -2.0) if u < 0.1 else (100.0, 100.0) if u < 0.15 else (50.0, 900.0)
                flipped, branches = int(rng.uniform() < 0.05), "7" if rng.uniform() > 0.05 else "7 12"
                f.write(f"{i};{bp};1;rs{i};{i // 10};{branches};0;{flipped};{begin:.6g};{end:.6g};{a}/{der};{a};{der};\n")
                if flipped == 0 and branches == "7" and begin < end:
                    searched.append((int(bp), a, der))
                for s in range(3):
                    if rng.uniform() < 0.85:
                        cnt = int(rng.integers(0, 4))
                        daf = int(rng.integers(0, cnt + 1))
                        ra, rd = (a, der) if rng.uniform() > 0.05 else (der, a)
                        recs[s].append((int(bp), ra, rd, cnt - daf, daf))
                    if rng.uniform() < 0.1:
                        recs[s].append((int(bp) + 1, "A", "G", 1, 1))
        for s in range(3):
            recs[s].sort(key=lambda r: r[0])
            for bp, ra, rd, aaf, daf in recs[s]:
                c = ch.encode()
                files[s].write(struct.pack("<i", len(c)) + c + struct.pack("<i", bp) + ra.encode() + rd.encode() + struct.pack("<ii", aaf, daf))
            bps = np.array([r[0] for r in recs[s]], dtype=np.int64)
            for bp, a, der in searched:  # the lower bound, the record in front of it, the counts where position and alleles match
                k = int(np.searchsorted(bps, bp, side="left"))
                prev = int(bps[k - 1]) if 0 < k < bps.size else -2
                hit = k < bps.size and recs[s][k][0] == bp and recs[s][k][1] == a and recs[s][k][2] == der
                idx[s].append((prev, recs[s][k][4] if hit else 0, recs[s][k][3] if hit else 0))
        r = np.zeros(len(searched), dtype=wl.ROW)
        r["pos"], r["age_begin"], r["age_end"] = [x[0] for x in searched], 1.0, 2.0
        rows.append(r)
        row_off.append(row_off[-1] + len(searched))
        first_pos.append(int(pos[0]))
        last_pos.append(int(pos[-1]))
    for f in files:
        f.close()
    with open(os.path.join(d, "chr.txt"), "w") as f:
        f.write("".join(c + "\n" for c in chroms))
    with open(os.path.join(d, "samples.txt"), "w") as f:
        f.write("".join(f"s{s} s{s}.colate.in\n" for s in range(3)))
    return dict(row_off=np.array(row_off, dtype=np.int64), rows=np.concatenate(rows), idx=np.array(idx, dtype=wl.IDX).reshape(3, -1),
                pairs=wl.make_pairs(ALL_PAIRS), first_pos=np.array(first_pos, dtype=np.int32), last_pos=np.array(last_pos, dtype=np.int32),
                window=BINSIZE)


def read_windows(path):
    """the two count columns of a pair's file"""
    out = [line.rsplit(" ", 2)[1:] for line in open(path).read().splitlines()]
    return np.array([[float(a), float(b)] for a, b in out]).T.astype(np.int32)


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


ENV_KEYS = ("COLATE_DEVICE_COMPARE", "COLATE_INDEXED_WALK", "COLATE_COMPARE_BUDGET")


def run_cli(d, args, env=None, timeout=120):
    """`Colate --mode compare_tmp ARGS` in d; env: COLATE_DEVICE_COMPARE and the like (those of the caller's are dropped)"""
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([il.CLI, "--mode", "compare_tmp"] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, env=e,
                          timeout=timeout)


HOST = {"COLATE_DEVICE_COMPARE": "0"}
CURSORS = {"COLATE_DEVICE_COMPARE": "0", "COLATE_INDEXED_WALK": "0"}


def assert_samples_files(d, meta, prefix):
    """every pair's file is the reference's, and PREFIX.pairs.txt holds the column sums in pair order"""
    lines = (d / f"{prefix}.pairs.txt").read_text().splitlines()
    assert len(lines) == len(meta["pairs"])
    for line, p in zip(lines, meta["pairs"]):
        t, r = p["names"]
        mine, want = (d / f"{prefix}_{t}_{r}.txt").read_bytes(), (d / p["output"]).read_bytes()
        assert len(want) > 100 and mine == want, (t, r)
        mm, n = read_windows(d / p["output"])
        assert line == f"{t} {r} {mm.sum()} {n.sum()}", (line, t, r)
