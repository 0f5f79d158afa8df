"""What the tests of colate_interval_fit_groups and of `Colate --mode mut_interval --pairs` share: the groups (record sets
of interval_cells_lib with block weights), the composition of the two single calls a grouped call has to equal bit for bit,
and the six-line pair list with its single runs."""

import numpy as np

import colate_amd
import interval_cells_lib as il
import synth_files

FIT = dict(max_iter=40, min_iter=10)


def with_weights(records, B, seed):
    """a group: the records and multinomial-looking block weights [B][nb] (whole numbers that sum to nb, some of them 0)"""
    nb = records[5]
    rng = np.random.default_rng(seed)
    bw = rng.multinomial(nb, np.full(nb, 1.0 / nb), size=B).astype(np.float64)
    return tuple(records) + (bw,)


def no_records(nb):
    z = np.zeros(0)
    return z.astype(np.float32), z.astype(np.float32), z, z, np.zeros(0, dtype=np.int32), nb


def all_beyond(n, nb):
    """records that all lie beyond the age grid: counted as dropped, no row"""
    blk = np.sort(np.arange(n, dtype=np.int32) % nb)
    return np.full(n, 100.0, dtype=np.float32), np.full(n, 3e7, dtype=np.float32), np.ones(n), np.ones(n), blk, nb


def one_per_cell(R, seed, nb=1):
    """R rows exactly: one record in each of the first R cells of the row order of kind 0 that lie past bin 40, with a shared
    weight only (so that no row of kind 1 appears)"""
    cells = [(bb, be) for bb in range(40, il.BINS) for be in range(bb, il.BINS)][:R]
    assert len(cells) == R
    rng = np.random.default_rng(seed)
    order = rng.permutation(R)  # (the records are not in row order)
    begin = np.array([il.age_in_bin(cells[i][0]) for i in order], dtype=np.float32)
    end = np.array([il.age_in_bin(cells[i][1]) for i in order], dtype=np.float32)
    blk = np.sort(rng.integers(0, nb, R).astype(np.int32))
    return begin, end, 10.0 ** rng.uniform(-2, 2, R), np.zeros(R), blk, nb


def composed(groups, epochs, device, math=1, init_rates=None, **fit):
    """per group interval_cells -> bootstrap_em_interval_batch: what interval_fit_groups has to return"""
    G, B = len(groups), groups[0][6].shape[0]
    ep = np.broadcast_to(np.asarray(epochs, dtype=np.float64), (G, np.asarray(epochs).shape[-1]))
    E = ep.shape[1]
    init = np.broadcast_to(np.full(E, colate_amd.DEFAULT_INIT_RATE) if init_rates is None else np.asarray(init_rates), (G, E))
    R, dropped = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int64)
    rates, iters, ll, flags = np.zeros((G, B, E)), np.zeros((G, B), dtype=np.int32), np.zeros((G, B)), np.zeros((G, B), dtype=np.int32)
    for g, grp in enumerate(groups):
        kinds, a0, a1, tables, dropped[g] = colate_amd.interval_cells(*grp[:6], device=device)
        R[g] = kinds.size
        if R[g] == 0:
            rates[g] = init[g]
            continue
        rates[g], iters[g], ll[g], flags[g] = colate_amd.bootstrap_em_interval_batch(
            kinds, a0, a1, grp[6], tables, ep[g], init_rates=init[g], device=device, math=math, **fit)
    return R, dropped, rates, iters, ll, flags


NAMES = ("R", "dropped", "rates", "iters", "loglik", "flags")


def assert_same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert il.same_bits(x, y), (name, x.shape, y.shape, np.argwhere(np.asarray(x) != np.asarray(y))[:5])


def epochs23():
    return colate_amd.epochs_from_bins("3,7,0.2")[0]


def four_groups(B=3):
    """G = 4 with nb = 1, 3, 5 and 2"""
    return [with_weights(il.random_records(60, 1, 21), B, 1), with_weights(il.random_records(40, 3, 22, empty=(1,)), B, 2),
            with_weights(il.random_records(30, 5, 23), B, 3), with_weights(il.random_records(50, 2, 24), B, 4)]


# ------------------------------------------------------------------ the command line
CLI_FIT = ["--num_bootstraps", "4", "--seed", "3", "--max_iter", "60", "--min_iter", "20"]
CLI_COMMON = ["--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2"]


def cli_inputs(d, **kw):
    """the synthetic files (cwd-relative names: T, T1, T2 x R, R1 over P_chr*.mut), a target mask and a .coal with another
    number of epochs"""
    kw = dict(dict(chroms=("1", "2"), snps_per_chr=1500, extra_targets=2, extra_refs=1), **kw)
    synth_files.write_inputs(str(d), **kw)
    for c in kw["chroms"]:
        il.write_mask(d / f"tm_chr{c}.fa", 20_000_000)
    ep = np.unique(colate_amd.epochs_from_bins("3,7,0.4")[0])  # (a .coal file's epochs increase strictly)
    colate_amd.write_coal(str(d / "warm.coal"), ep, np.full((1, ep.size), 2e-5))


# (target, reference, output, further tokens of the list line, the same as options of the single run)
SIX_PAIRS = [("T.colate.in", "R.colate.in", "p1", [], []),
             ("T1.colate.in", "R.colate.in", "p2", [], []),
             ("T.colate.in", "R.colate.in", "p3", ["target_mask=tm"], ["--target_mask", "tm"]),
             ("T2.colate.in", "R1.colate.in", "p4", ["coal=warm.coal"], ["--coal", "warm.coal"]),
             ("T.colate.in", "R.colate.in", "p5", [], []),  # the first pair again, under another name
             ("T1.colate.in", "R1.colate.in", "p6", [], [])]


def write_list(path, pairs, prefix=""):
    with open(path, "w") as f:
        for t, r, out, extra, _ in pairs:
            f.write(" ".join([t, r, prefix + out] + extra) + "\n")


def run_pairs(d, list_name, device, more=(), fit=CLI_FIT, common=CLI_COMMON):
    return il.run_cli(["--pairs", list_name] + list(common) + list(fit) + list(more), d, device=device)


def run_single(d, pair, out, device, fit=CLI_FIT):
    t, r, _, _, opts = pair
    common = [a for a in CLI_COMMON if not (opts[:1] == ["--coal"] and a in ("--bins", "3,7,0.2"))]
    return il.run_cli(common + ["--target_tmp", t, "--reference_tmp", r, "-o", out] + opts + list(fit), d, device=device)


def pair_lines(stderr, i, P):
    """the lines of pair i of P on the stderr of a --pairs run without their `Pair i` prefixes: `Number of blocks: n`,
    `Number of rows: n`, `SNPs beyond the age grid: n` and the `Bootstrap k: Total iterations n` lines, in order"""
    head, out = f"Pair {i} / {P}: ", []
    for line in stderr.splitlines():
        if line.startswith(head) and "Number of blocks: " in line:
            out.append(line[line.index("Number of blocks: "):])
        elif line.startswith(f"Pair {i} Number of rows: ") or line.startswith(f"Pair {i} SNPs beyond") or line.startswith(f"Pair {i} Bootstrap "):
            out.append(line[len(f"Pair {i} "):])
    return out


def single_lines(stderr):
    return [line for line in stderr.splitlines() if line.startswith(("Number of blocks: ", "Number of rows: ", "SNPs beyond", "Bootstrap "))]
