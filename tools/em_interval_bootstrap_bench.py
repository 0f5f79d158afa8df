"""Measures the block bootstrap in front of the interval-dated EM fit at --bins 3,7,0.2: R = 370 rows (the 185 grid ages,
shared and not-shared, each dated to the interval from its grid age to the age three bins on), nb = 115 genome blocks with
Poisson counts per block and row, B = 100 replicates with multinomial block weights, run to the reference's stop rule
(max_iter 100000, min_iter 1000, rel_tol 1e-7).

After one warm-up each, as the median of --reps runs (wall clock around the synchronous calls):
  * bootstrap_call: colate_bootstrap_em_interval_batch -- tables and block weights in, the weighted block sums W formed by
    the bootstrap kernel and left in device memory for the fit;
  * host_sums_then_fit (the baseline, what a caller did before): W = block_weights @ tables in numpy on the host, then
    colate_em_interval_batch, which copies the B x R matrix to the device.
numpy's product may sum in another order than the contract's, so the baseline's rates need not be the call's bit for bit;
`bit_identical_to_contract_order` compares the call with colate_em_interval_batch on colate_bootstrap_rows_host's sums,
`bit_identical_to_numpy_baseline` with the baseline as timed.  Nothing is gated: the fit dominates both, the difference
is the B x R round trip.

Prints one JSON document and writes it to --record (default profiles/interval/em_interval_bootstrap_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import colate_amd  # noqa: E402
from colate_amd.api import DEFAULT_MAX_ITER, DEFAULT_MIN_ITER, DEFAULT_REL_TOL  # noqa: E402


def problem(B, nb, seed=3):
    rng = np.random.default_rng(seed)
    grid = colate_amd.age_grid()
    ep, _ = colate_amd.epochs_from_bins("3,7,0.2")
    later = grid[np.minimum(np.arange(grid.size) + 3, grid.size - 1)]
    kinds = np.tile([0, 1], grid.size).astype(np.int32)
    a0, a1 = np.repeat(grid, 2), np.repeat(later, 2)
    # mean counts per block that fall off with age on both sides of a mode, as a genome's age spectrum does
    mean = 40.0 / nb * np.exp(-0.5 * ((np.log(np.maximum(np.repeat(grid, 2), 1.0)) - np.log(3e3)) / 2.0) ** 2)
    tables = rng.poisson(mean, (nb, kinds.size)).astype(float)
    bw = colate_amd.bootstrap_weights(colate_amd.Rng(seed), B, nb)
    return kinds, a0, a1, bw, tables, ep


def timed(f, reps):
    res = f()  # warm-up: code objects, workspace, caches
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        res = f()
        walls.append(time.perf_counter() - t)
    return res, walls


def record(walls, iters):
    return {"iterations_total": int(np.sum(iters)), "wall_s_median": round(statistics.median(walls), 5),
            "wall_s_all": [round(x, 5) for x in walls]}


def same_bits(x, y):
    return bool(all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(x, y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "interval", "em_interval_bootstrap_bench.json"))
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=115)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=DEFAULT_MAX_ITER)
    ap.add_argument("--min-iter", type=int, default=DEFAULT_MIN_ITER)
    a = ap.parse_args()
    assert a.reps >= 3, "the median of at least 3 runs"
    k, a0, a1, bw, t, ep = problem(a.replicates, a.blocks)
    fit = dict(max_iter=a.max_iter, min_iter=a.min_iter)
    out = {"input": f"--bins 3,7,0.2 (E = {ep.size}), R = {k.size}, B = {a.replicates}, nb = {a.blocks}, max_iter {a.max_iter}, "
                    f"min_iter {a.min_iter}, rel_tol {DEFAULT_REL_TOL}", "reps": a.reps}
    new, walls = timed(lambda: colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, **fit), a.reps)
    out["bootstrap_call"] = record(walls, new[1])
    print(json.dumps({"bootstrap_call": out["bootstrap_call"]}), flush=True)
    old, walls = timed(lambda: colate_amd.em_interval_batch(k, a0, a1, bw @ t, ep, **fit), a.reps)
    out["host_sums_then_fit"] = record(walls, old[1])
    contract = colate_amd.em_interval_batch(k, a0, a1, colate_amd.bootstrap_rows(bw, t), ep, **fit)
    out["bit_identical_to_contract_order"] = same_bits(new, contract)
    out["bit_identical_to_numpy_baseline"] = same_bits(new, old)
    out["numpy_sums_equal_contract_sums"] = same_bits([bw @ t], [colate_amd.bootstrap_rows(bw, t)])
    out["bootstrap_call_over_baseline"] = round(out["bootstrap_call"]["wall_s_median"] / out["host_sums_then_fit"]["wall_s_median"], 4)
    s = json.dumps(out, indent=1)
    print(s)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
