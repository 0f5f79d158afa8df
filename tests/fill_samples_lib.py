"""What the tests of colate_fill_samples and of `Colate --mode mut --samples` share: the cases beyond those of
interval_walk_lib (the row-0 kernel's batch edges, the jobs kernel's segments, a pair that is handed back), the comparison of
two fills bit for bit, the chunk rule restated, and the command line with its lists."""
import concurrent.futures
import functools
import os
import subprocess

import numpy as np

import colate_amd
import golden_lib as gl
import interval_cells_lib as il
import interval_walk_lib as wl
import pairs_masks_lib as pm

SEED = 11
A = 185
ROW, IDX = wl.ROW, wl.IDX
REC_BYTES = 40  # a record of the fill and its row-0 weights on the device


def fill(c, device, seed=SEED, **kw):
    return colate_amd.fill_samples(c["row_off"], c["rows"], c["idx"], c["masks"], c["pairs"], c["nbpb"], seed, device=device, **kw)


def assert_same_fill(got, want):
    """nb, used, words and every table equal in every bit"""
    for k in ("nb", "used", "words"):
        assert il.same_bits(got[k], want[k]), (k, got[k], want[k])
    assert len(got["tables"]) == len(want["tables"])
    for p, (x, y) in enumerate(zip(got["tables"], want["tables"])):
        assert x.shape == y.shape and il.same_bits(x, y), (p, x.shape, np.argwhere(x.view(np.uint64) != y.view(np.uint64))[:5])


def all_used(n_samples, pos, age_begin, age_end, rng):
    """one chromosome in which every pair of different samples uses every row: each index entry points just in front of its
    row and carries both alleles"""
    n = len(pos)
    rows = np.zeros(n, dtype=ROW)
    rows["pos"], rows["age_begin"], rows["age_end"] = pos, age_begin, age_end
    idx = np.zeros((n_samples, n), dtype=IDX)
    for s in range(n_samples):
        idx[s]["prev_bp"] = rows["pos"] - 1
        idx[s]["DAF"], idx[s]["AAF"] = rng.integers(1, 4, n), rng.integers(1, 3, n)
    return np.array([0, n], dtype=np.int64), rows, idx


def bin_centre(k):
    """an age in the middle of age bin k (1 <= k < A)"""
    return np.float32(np.exp((k - 1) / 10.0) / 10.0)


def frow_sizes_case():
    """blocks of 1000 bases holding 63, 64, 65 and 129 F records (age_begin 0.0, -0.0 and negative in turn, ends all over the
    grid) with a non-F record now and then, one F record ending beyond the grid, and a last block without an F record"""
    rng = np.random.default_rng(21)
    pos, ab, ae = [], [], []
    for k, n_f in enumerate([63, 64, 65, 129, 0]):
        at = k * 1000 + 1
        for i in range(n_f):
            pos.append(at), ab.append([0.0, -0.0, -3.5][i % 3]), ae.append(bin_centre(int(rng.integers(20, 170))))
            at += 1
            if i % 17 == 5:  # a non-F record inside the batch
                pos.append(at), ab.append(120.0), ae.append(260.0)
                at += 1
        if k == 2:
            ae[-1] = np.float32(3e7)  # beyond the grid: nothing for row 0, and only its samples below the grid's end count
        if n_f == 0:
            for i in range(10):
                pos.append(at + i), ab.append(50.0 + i), ae.append(130.0 + i)
    row_off, rows, idx = all_used(2, pos, np.array(ab, dtype=np.float32), np.array(ae, dtype=np.float32), rng)
    return wl.case(row_off, rows, idx, wl.make_pairs([(0, 1), (1, 0)]), 1000)


def frow_bins_case():
    """two blocks of exactly one batch each: 64 F records that all end in one bin, and 64 that end in 64 different bins"""
    rng = np.random.default_rng(22)
    pos = np.concatenate([1 + np.arange(64), 1001 + np.arange(64)])
    ae = np.concatenate([np.full(64, bin_centre(90)), [bin_centre(60 + i) for i in range(64)]]).astype(np.float32)
    row_off, rows, idx = all_used(2, pos, np.zeros(128, dtype=np.float32), ae, rng)
    return wl.case(row_off, rows, idx, wl.make_pairs([(0, 1)]), 1000)


def jobs_case():
    """520 rows at positions 1 .. 520 with one base per block: the pair of samples 0 and 1 has 520 one-row blocks (more than
    the 512 tables per pair of the `--pairs` engine's device path); sample 2 never carries a derived allele, so the pair
    that has it as reference uses no row at all"""
    rng = np.random.default_rng(23)
    n = 520
    ab = (10.0 ** rng.uniform(1, 3, n)).astype(np.float32)
    ab[::7] = 0.0
    row_off, rows, idx = all_used(3, 1 + np.arange(n), ab, (np.maximum(ab, 30.0) * 1.8).astype(np.float32), rng)
    idx[2]["DAF"] = 0
    return wl.case(row_off, rows, idx, wl.make_pairs([(0, 1), (0, 2), (1, 0)]), 1)


def hand_back_case():
    """two pairs side by side over 300 rows in two blocks: only sample 1 carries a derived allele at row 150, a non-F row
    whose ages run from inside the grid to beyond it -- the pair with sample 1 as reference draws again there; the other is clean"""
    rng = np.random.default_rng(24)
    n = 300
    ab = (10.0 ** rng.uniform(1, 3, n)).astype(np.float32)
    ab[::5] = 0.0
    ae = (np.maximum(ab, 30.0) * 2.0).astype(np.float32)
    ab[150], ae[150] = 5e6, 2e7
    row_off, rows, idx = all_used(3, 1 + 7 * np.arange(n), ab, ae, rng)
    idx[2]["DAF"][150] = 0
    return wl.case(row_off, rows, idx, wl.make_pairs([(0, 1), (0, 2)]), 1500)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case; every case but hand_back is meant to stay on the device"""
    c = dict(wl.cases())
    c.update(frow_sizes=frow_sizes_case(), frow_bins=frow_bins_case(), jobs=jobs_case(), hand_back=hand_back_case())
    return c


HANDED_BACK = {"hand_back": [1, 0]}  # near_band of every other case is all zero (test_fill_samples_cpu checks it)


@functools.lru_cache(maxsize=None)
def twin(name):
    return fill(cases()[name], device=False)


def chunks_by_rule(used, budget_mb):
    """runs of consecutive pairs whose records fit the budget; a larger pair goes alone"""
    budget = max(1, budget_mb * (1 << 20) // REC_BYTES)
    n, p0 = 0, 0
    while p0 < len(used):
        p1, recs = p0 + 1, int(used[p0])
        while p1 < len(used) and recs + int(used[p1]) <= budget:
            recs += int(used[p1])
            p1 += 1
        n, p0 = n + 1, p1
    return n


# ------------------------------------------------------------------ the command line
ENV_KEYS = ("COLATE_DEVICE_FILL", "COLATE_DEVICE_FILL_WALK", "COLATE_INDEXED_WALK", "COLATE_TIMING", "COLATE_FILL_SAMPLES_RECS_MB")


def run_cli(d, args, env=None, timeout=300):
    e = dict(os.environ)
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([il.CLI, "--mode", "mut", "--mut", "P"] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True,
                          env=e, timeout=timeout)


def expand(samples):
    """the `--pairs` lines of a sample list given as (name, file, mask or None, role or None, age or None): (output suffix, line)"""
    out = []
    for t in samples:
        for r in samples:
            if t is r or t[3] == "reference" or r[3] == "target":
                continue
            toks = [t[1], r[1], f"{t[0]}_{r[0]}", t[4] or "0", r[4] or "0"]
            toks += [f"target_mask={t[2]}"] if t[2] else []
            toks += [f"reference_mask={r[2]}"] if r[2] else []
            out.append((f"{t[0]}_{r[0]}", toks))
    return out


def sample_lines(samples):
    return [" ".join([s[0], s[1]] + ([f"mask={s[2]}"] if s[2] else []) + ([f"role={s[3]}"] if s[3] else []) + ([f"age={s[4]}"] if s[4] else []))
            for s in samples]


# the fixtures as sample lists: (fixture, stage function, lists); a list is its samples and {output suffix: fixture pair}
L3_LISTS = [  # T1 is 500 years old in two pairs of l3_pairs and 7000 in one: two lists
    ([("T", "T.colate.in", None, None, None), ("T1", "T1.colate.in", None, None, "500"), ("R", "R.colate.in", None, None, None),
      ("R1", "R1.colate.in", None, None, None)], {"T_R": "p0", "T1_R": "p1", "T_R1": "p2", "R_T": "p4", "R1_T1": "p5"}),
    ([("T1", "T1.colate.in", None, "target", "7000"), ("R1", "R1.colate.in", None, "reference", None)], {"T1_R1": "p3"}),
]
MASK_LISTS = [
    ([("T", "T.colate.in", "TM", "target", None), ("R", "R.colate.in", "RM", "reference", None),
      ("R1", "R1.colate.in", "RM1", "reference", None)], {"T_R": "p0", "T_R1": "p3"}),
    ([("T1", "T1.colate.in", "TM1", "target", None), ("T", "T.colate.in", None, "target", None), ("R", "R.colate.in", None, "reference", None),
      ("R1", "R1.colate.in", None, "reference", None)], {"T1_R": "p1", "T_R1": "p2"}),
]
FIXTURES = {"l3_pairs": (gl.l3_pairs_stage, L3_LISTS), "pairs_masks": (pm.stage, MASK_LISTS)}


def run_many(d, runs):
    """run_cli for every (args, env) of `runs`, side by side (each writes files of its own): the completed processes in order"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, len(runs))) as pool:
        return list(pool.map(lambda r: run_cli(d, r[0], r[1]), runs))


def write_lists(d, samples, k):
    """samples<k>.txt and its expansion expanded<k>.txt (outputs e<k>_*); returns the output suffixes of the pairs"""
    (d / f"samples{k}.txt").write_text("\n".join(sample_lines(samples)) + "\n")
    ex = expand(samples)
    (d / f"expanded{k}.txt").write_text("".join(" ".join([t[0], t[1], f"e{k}_{t[2]}"] + t[3:]) + "\n" for _, t in ex))
    return [name for name, _ in ex]


def both_runs(common, k, more=(), env=None):
    """`--samples` on list k (outputs s<k>_*) and `--pairs` on its expansion, as (args, env) for run_many"""
    return [(list(common) + ["--samples", f"samples{k}.txt", "-o", f"s{k}"] + list(more), env),
            (list(common) + ["--pairs", f"expanded{k}.txt"] + list(more), dict(env or {}, COLATE_TIMING="1"))]


def run_both(d, common, samples, k, more=(), env=None):
    """the two completed processes of both_runs and the output suffixes"""
    names = write_lists(d, samples, k)
    rs, rp = run_many(d, both_runs(common, k, more, env))
    return rs, rp, names


def assert_all_indexed(rp, n_pairs):
    """the `--pairs` run's timing line: every pair walked through the files' indices (else the fixture cannot reach the device path)"""
    assert rp.returncode == 0, rp.stderr[-800:]
    assert f"{n_pairs} of {n_pairs} pairs walked through indices" in rp.stderr, rp.stderr[-1500:]
