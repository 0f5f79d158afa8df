"""What the tests of colate_interval_walk / colate_interval_fit_samples and of `Colate --mode mut_interval --samples` share:
the walk contract restated as a plain Python loop over numpy arrays (independent of the C++), and the case builder used on
both machines.  W is the tile width the kernel exports; the cases sit on its edges."""
import functools
import os
import subprocess

import numpy as np

import colate_amd
import interval_cells_lib as il
import interval_groups_lib as gl

ROW, IDX, PAIR, REC = colate_amd.WALK_ROW, colate_amd.WALK_IDX, colate_amd.WALK_PAIR, colate_amd.INTERVAL_REC
W = colate_amd.interval_walk_tile()


# ------------------------------------------------------------------ the contract, as a loop
def block_of_pos(pos, nbpb):
    base, k = 0, 0
    while base + nbpb < pos:
        base += nbpb
        k += 1
    return k


def record(row, t, r):
    """a used row as (begin, end, w_sh, w_ns): the float product, the conversion and the double division rounded apiece"""
    ab = float(row["age_begin"])
    if ab < 0.0:
        ab = 0.0
    n_t = int(t["DAF"]) + int(t["AAF"])
    n_r = int(r["DAF"]) + int(r["AAF"])

    def call(count):  # roundf of the float quotient: halves away from zero (the quotient is not negative)
        f = np.float32(np.float64(np.float32(count)) / (n_t / 2.0))
        return np.float32(np.floor(np.float64(f) + 0.5))

    daf_r = np.float32(int(r["DAF"]))
    w_sh = np.float64(np.float32(call(int(t["DAF"])) * daf_r)) / np.float64(n_r)
    w_ns = np.float64(np.float32(call(int(t["AAF"])) * daf_r)) / np.float64(n_r)
    return np.float32(ab), row["age_end"], w_sh, w_ns


def mask_bit(masks, word_off, m, c, i):
    return m < 0 or (int(masks[m, word_off[c] + (i >> 6)]) >> (i & 63)) & 1


def model(case):
    """(rec_off, nb, recs, block) of a case, pair by pair, chromosome by chromosome, row by row"""
    row_off, rows, idx, masks, pairs, nbpb = (case[k] for k in ("row_off", "rows", "idx", "masks", "pairs", "nbpb"))
    C = len(row_off) - 1
    word_off = np.concatenate([[0], np.cumsum((np.diff(row_off) + 63) // 64)]).astype(np.int64)
    recs, blocks, rec_off, nbs = [], [], [0], []
    for pr in pairs:
        tg, rf, tm, rm = (int(pr[k]) for k in ("target", "reference", "target_mask", "reference_mask"))
        nb = 0
        for c in range(C):
            lo, n = int(row_off[c]), int(row_off[c + 1] - row_off[c])
            rr, TI, RI = rows[lo:lo + n], idx[tg, lo:lo + n], idx[rf, lo:lo + n]
            pos = lambda i: -1 if i < 0 else int(rr[i]["pos"])  # noqa: E731
            searched = ref_pass = -1
            last_k = -1
            for i in range(n):
                if not (mask_bit(masks, word_off, tm, c, i) and mask_bit(masks, word_off, rm, c, i)):
                    continue
                ref_from, searched = searched, i
                if RI[i]["DAF"] == 0 or int(RI[i]["prev_bp"]) < pos(ref_from):
                    continue
                tgt_from, ref_pass = ref_pass, i
                if (int(TI[i]["DAF"]) | int(TI[i]["AAF"])) == 0 or int(TI[i]["prev_bp"]) < pos(tgt_from):
                    continue
                last_k = block_of_pos(int(rr[i]["pos"]), nbpb)
                recs.append(record(rr[i], TI[i], RI[i]))
                blocks.append(nb + last_k)
            nb += last_k + 1 if last_k >= 0 else 1
        nbs.append(nb)
        rec_off.append(len(recs))
    out = np.zeros(len(recs), dtype=REC)
    for j, (b, e, s, n_) in enumerate(recs):
        out[j] = (b, e, s, n_)
    return np.array(rec_off, dtype=np.int64), np.array(nbs, dtype=np.int32), out, np.array(blocks, dtype=np.int32)


# ------------------------------------------------------------------ the cases
FIVE_PAIRS = [(0, 1), (1, 2), (0, 1), (2, 2), (2, 0)]  # over three samples: one pair twice, one with target = reference


def make_pairs(tr, masks=None):
    p = np.zeros(len(tr), dtype=PAIR)
    for j, (t, r) in enumerate(tr):
        p[j] = (t, r) + (tuple(masks[j]) if masks else (-1, -1))
    return p


def make_rows(ns, rng, step=40):
    """ascending positions (about one pair in ten equal), age_begin < age_end, a tenth of the lower ages negative"""
    rows, row_off = [], [0]
    for n in ns:
        r = np.zeros(n, dtype=ROW)
        r["pos"] = 1 + np.cumsum(rng.integers(0, step, n) * (rng.uniform(size=n) > 0.1))
        a0 = (10.0 ** rng.uniform(1, 3, n)).astype(np.float32)
        a0[rng.uniform(size=n) < 0.1] *= -1
        a0[rng.uniform(size=n) < 0.05] = 0.0
        r["age_begin"], r["age_end"] = a0, (np.maximum(a0, 30.0) * (1 + 1.5 * rng.uniform(size=n))).astype(np.float32)
        rows.append(r)
        row_off.append(row_off[-1] + n)
    return np.array(row_off, dtype=np.int64), np.concatenate(rows)


def make_idx(S, row_off, rows, rng, zero=0.15):
    """prev_bp on, one below and one above the position of the row in front (the `<` of the rule, where that row was the
    latest search), sometimes further back, sometimes -2; counts 0 .. 4 with zeros"""
    n = rows.size
    idx = np.zeros((S, n), dtype=IDX)
    prev = np.concatenate([[-1], rows["pos"][:-1]]).astype(np.int64)
    prev[row_off[:-1][np.diff(row_off) > 0]] = -1  # a chromosome's first row: pos(-1)
    back = np.concatenate([[-1, -1, -1], rows["pos"]])[:n].astype(np.int64)
    for s in range(S):
        u = rng.uniform(size=n)
        pb = prev + rng.integers(-1, 2, n)
        pb = np.where(u < 0.25, back + rng.integers(-1, 2, n), pb)
        pb = np.where(u > 0.93, -2, pb)
        idx[s]["prev_bp"] = np.maximum(pb, -2)
        idx[s]["DAF"] = rng.integers(0, 5, n) * (rng.uniform(size=n) > zero)
        idx[s]["AAF"] = rng.integers(0, 5, n) * (rng.uniform(size=n) > zero)
    return idx


def case(row_off, rows, idx, pairs, nbpb, masks=None):
    words = int(((np.diff(row_off) + 63) // 64).sum())
    masks = np.zeros((0, words), dtype=np.uint64) if masks is None else masks
    return dict(row_off=row_off, rows=rows, idx=idx, masks=masks, pairs=pairs, nbpb=nbpb)


def random_case(ns, seed, nbpb=3000, S=3, tr=FIVE_PAIRS, step=40):
    rng = np.random.default_rng(seed)
    row_off, rows = make_rows(ns, rng, step)
    return case(row_off, rows, make_idx(S, row_off, rows, rng), make_pairs(tr), nbpb)


def bits(flags_per_chr):
    """a mask's words from one array of 0 / 1 per chromosome, each chromosome starting on a word"""
    out = []
    for f in flags_per_chr:
        w = np.zeros((len(f) + 63) // 64, dtype=np.uint64)
        for i in np.flatnonzero(f):
            w[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        out.append(w)
    return np.concatenate(out)


def carry_case():
    """reference-passing rows only in the first and in the last of four tiles: the carry crosses two tiles that have none; the
    target index of the last-tile row points on (sample 0) and one below (sample 2) the position of the first-tile row"""
    rng = np.random.default_rng(5)
    row_off, rows = make_rows([4 * W], rng)
    rows["pos"] = 10 + 3 * np.arange(4 * W)
    idx = make_idx(3, row_off, rows, rng)
    a, b = 7, 3 * W + 9
    idx[1]["DAF"] = 0
    for i in (a, a + 1, b, b + 1):
        idx[1][i] = (rows["pos"][i] - 1, 2, 1)  # passes as reference: prev_bp >= the row in front
    for s, d in ((0, 0), (2, -1)):
        idx[s][a] = (-2 if s == 2 else rows["pos"][a] - 1, 1, 1)
        idx[s][a + 1] = (rows["pos"][a] + d, 1, 2)
        idx[s][b] = (rows["pos"][a + 1] + d, 2, 1)
        idx[s][b + 1] = (rows["pos"][b] + d, 1, 1)
    return case(row_off, rows, idx, make_pairs([(0, 1), (2, 1), (1, 1)]), 400)


def mask_case():
    """chromosomes of 3W and W + 70 rows (mask words ending mid-word) and one of 5; mask 0 removes the whole second tile of the
    first chromosome, mask 1 every row, mask 2 is random, mask 3 removes nothing"""
    rng = np.random.default_rng(6)
    ns = [3 * W, W + 70, 5]
    row_off, rows = make_rows(ns, rng)
    idx = make_idx(3, row_off, rows, rng, zero=0.05)
    m0 = [np.ones(n, dtype=int) for n in ns]
    m0[0][W:2 * W] = 0
    m0[1][::3] = 0
    masks = np.stack([bits(m0), bits([np.zeros(n, dtype=int) for n in ns]), bits([rng.integers(0, 2, n) for n in ns]),
                      bits([np.ones(n, dtype=int) for n in ns])])
    pairs = make_pairs([(0, 1), (0, 1), (0, 1), (0, 1), (1, 0), (2, 1)], [(0, -1), (-1, 0), (0, 2), (1, -1), (-1, -1), (3, 2)])
    return case(row_off, rows, idx, pairs, 2500, masks)


def equal_positions_case():
    """four rows at one position on each side of the first tile edge, and a run of equal positions across the second"""
    c = random_case([3 * W + 5], 7)
    c["rows"]["pos"][W - 2:W + 2] = c["rows"]["pos"][W - 2]
    c["rows"]["pos"][2 * W - 5:2 * W + 6] = c["rows"]["pos"][2 * W - 5]
    assert (np.diff(c["rows"]["pos"]) >= 0).all()
    c["idx"] = make_idx(3, c["row_off"], c["rows"], np.random.default_rng(8))
    return c


def counts_case():
    """every row used: target counts on the half-way rounding (1,3; 3,1; 1,2; 65535,0 ...), reference counts up to 65535, a
    negative age_begin"""
    tgt = [(1, 3), (3, 1), (1, 2), (65535, 0), (0, 65535), (2, 2), (1, 1), (5, 3), (3, 5), (1, 0), (0, 1), (65535, 65535), (7, 1)]
    ref = [(1, 1), (2, 0), (1, 3), (65535, 1), (3, 65535), (65535, 65535), (1, 0), (2, 1), (1, 2), (4, 4), (3, 1), (1, 1), (6, 2)]
    n = len(tgt)
    rows = np.zeros(n, dtype=ROW)
    rows["pos"] = 100 + 10 * np.arange(n)
    rows["age_begin"] = np.array([-5.0, 0.0, 12.5] + [100.0 + i for i in range(n - 3)], dtype=np.float32)
    rows["age_end"] = rows["age_begin"] + np.float32(250.0)
    rows["age_end"][0] = 40.0
    idx = np.zeros((2, n), dtype=IDX)
    for i in range(n):
        idx[0][i] = (rows["pos"][i] - 5, tgt[i][0], tgt[i][1])
        idx[1][i] = (rows["pos"][i] - 5, ref[i][0], ref[i][1])
    return case(np.array([0, n], dtype=np.int64), rows, idx, make_pairs([(0, 1), (1, 0), (0, 0)]), 50)


def blocks_case(nbpb=100):
    """three chromosomes, the middle one without a used row (no sample carries a derived allele there); positions over four
    blocks of which one holds no row"""
    rng = np.random.default_rng(9)
    ns = [40, 30, 50]
    row_off, rows = make_rows(ns, rng)
    for c, n in enumerate(ns):
        k = rng.choice([0, 1, 3], n)  # (block 2 stays empty)
        rows["pos"][row_off[c]:row_off[c + 1]] = np.sort(1 + k * nbpb + rng.integers(0, nbpb, n))
    idx = make_idx(3, row_off, rows, rng, zero=0.05)
    for s in range(3):
        idx[s]["DAF"][row_off[1]:row_off[2]] = 0
    return case(row_off, rows, idx, make_pairs(FIVE_PAIRS), nbpb)


def one_base_blocks_case():
    """num_bases_per_block = 1: a block per position"""
    c = random_case([60, 1, 45], 10, nbpb=1, step=3)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case"""
    c = {"sizes": random_case([1, W - 1, W, W + 1, 3 * W + 5], 1),  # rows per chromosome on the edges of the tile
         "one_row": random_case([1], 2, tr=[(0, 1), (1, 0), (2, 2)]),
         "carry": carry_case(), "masks": mask_case(), "equal_positions": equal_positions_case(), "counts": counts_case(),
         "blocks": blocks_case(), "one_base_blocks": one_base_blocks_case()}
    return c


@functools.lru_cache(maxsize=None)
def modelled(name):
    return model(cases()[name])


def walk(c, device, cap=None):
    return colate_amd.interval_walk(c["row_off"], c["rows"], c["idx"], c["masks"], c["pairs"], c["nbpb"], device=device, cap=cap)


WALK_NAMES = ("rec_off", "nb", "recs", "block")


def assert_same_walk(got, want):
    for name, x, y in zip(WALK_NAMES, got, want):
        assert il.same_bits(x, y), (name, x.shape, y.shape, x[:8], y[:8])


# ------------------------------------------------------------------ the fit
FIT_NAMES = ("nb", "used") + gl.NAMES
SEED, B = 11, 3


def fit_samples(c, device, seed=SEED, num_bootstrap=B, **fit):
    fit = dict(gl.FIT, **fit)
    return colate_amd.interval_fit_samples(c["row_off"], c["rows"], c["idx"], c["masks"], c["pairs"], c["nbpb"], num_bootstrap,
                                           gl.epochs23(), seed, device=device, **fit)


def fit_groups_on(walked, device, seed=SEED, num_bootstrap=B, **fit):
    """interval_fit_groups on the records of a walk, every pair's weights from a fresh generator on the seed"""
    fit = dict(gl.FIT, **fit)
    rec_off, nb, recs, block = walked
    groups = []
    for p in range(nb.size):
        r, blk = recs[rec_off[p]:rec_off[p + 1]], block[rec_off[p]:rec_off[p + 1]]
        bw = colate_amd.bootstrap_weights(colate_amd.Rng(seed), num_bootstrap, int(nb[p]))
        groups.append((r["begin"], r["end"], r["w_sh"], r["w_ns"], blk, int(nb[p]), bw))
    return (nb, np.diff(rec_off)) + tuple(colate_amd.interval_fit_groups(groups, gl.epochs23(), device=device, **fit))


def assert_same_fit(got, want):
    for name, x, y in zip(FIT_NAMES, got, want):
        assert il.same_bits(np.asarray(x), np.asarray(y)), (name, np.asarray(x).shape, np.asarray(y).shape)


def many_records_case():
    """five pairs of 15 000 records and more in 1, 1, 1, 3 and 1 blocks: a megabyte of records (28 bytes each) holds two
    pairs, a megabyte of dense cell sums three segments.  Only sample 3 carries a derived allele at the ten far rows, so only
    the pair that has it as reference reaches the third block (the second holds no row)."""
    rng = np.random.default_rng(12)
    near, far = 15000, 10
    n = near + far
    row_off, rows = make_rows([n], rng)
    rows["pos"] = np.concatenate([1 + np.arange(near), 2 * near + 1 + np.arange(far)])
    idx = np.zeros((4, n), dtype=IDX)
    for s in range(4):
        idx[s]["prev_bp"] = rows["pos"] - 1  # (at or behind the row in front: every search moves)
        idx[s]["DAF"], idx[s]["AAF"] = rng.integers(1, 4, n), rng.integers(0, 3, n)
        if s < 3:
            idx[s]["DAF"][near:], idx[s]["AAF"][near:] = 0, 1
    return case(row_off, rows, idx, make_pairs([(0, 1), (1, 2), (2, 0), (0, 3), (1, 0)]), near)


# ------------------------------------------------------------------ the command line
def run_samples_cli(d, list_name, out, device, more=(), env=None, fit=gl.CLI_FIT, common=gl.CLI_COMMON, timeout=120):
    """`Colate --mode mut_interval --samples LIST -o OUT` in d; device=False: COLATE_DEVICE_INTERVAL=0; env: further variables"""
    e = dict(os.environ)
    for k in ("COLATE_DEVICE_INTERVAL", "COLATE_DEVICE_INTERVAL_WALK", "COLATE_INDEXED_WALK"):
        e.pop(k, None)
    if not device:
        e["COLATE_DEVICE_INTERVAL"] = "0"
    e.update(env or {})
    args = ["--mode", "mut_interval", "--samples", list_name, "-o", out] + list(common) + list(fit) + [str(a) for a in more]
    return subprocess.run([il.CLI] + args, cwd=str(d), capture_output=True, text=True, env=e, timeout=timeout)


# the list of the tests (a role= split, a masked sample that is target and reference, a blank line) and its expansion as a
# `--pairs` list: (target, reference, output, further tokens of the list line, the same as options of the single run)
SAMPLES = ["a T.colate.in role=target", "", "b T1.colate.in mask=tm", "c R.colate.in role=reference", "d R1.colate.in role=reference"]
EXPANDED = [("T.colate.in", "T1.colate.in", "a_b", ["reference_mask=tm"], ["--reference_mask", "tm"]),
            ("T.colate.in", "R.colate.in", "a_c", [], []),
            ("T.colate.in", "R1.colate.in", "a_d", [], []),
            ("T1.colate.in", "R.colate.in", "b_c", ["target_mask=tm"], ["--target_mask", "tm"]),
            ("T1.colate.in", "R1.colate.in", "b_d", ["target_mask=tm"], ["--target_mask", "tm"])]


def run_samples(d, lines, out, device, more=(), env=None):
    (d / "samples.txt").write_text("\n".join(lines) + "\n")
    return run_samples_cli(d, "samples.txt", out, device, more, env)
