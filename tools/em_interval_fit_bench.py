"""Measures the EM fit on interval-dated mutations (colate_em_interval_batch) at --bins 3,7,0.2: R = 370 rows -- the 185
grid ages, shared and not-shared, each dated to the interval from its grid age to the age three bins on -- B = 100
replicates with Poisson weights, run to the reference's stop rule (max_iter 100000, min_iter 1000, rel_tol 1e-7).

After one warm-up each, as the median of --reps runs (wall clock around the synchronous call):
  * device_call: colate_em_interval_batch, the whole loop in one launch;
  * host_driven_loop: the same fit driven from the host, one colate_em_interval_calls (weights given) per iteration plus
    the M-step and stop rule in numpy -- what a caller could do before -- over the first --loop-replicates replicates
    (the replicates are independent and run one after the other, so the time per replicate is what scales);
  * host_twin: colate_em_interval_batch_host with math = 1 over the first --host-replicates replicates.
Every entry records its replicates, seconds per run and seconds per replicate; the device's results are compared with
the host twin's (bit for bit) and the host-driven loop's on the replicates they share.

Prints one JSON document and writes it to --record (default profiles/interval/em_interval_fit_bench.json).
--host-only: no device runs (a machine without a GPU): only host_twin is measured."""
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
from colate_amd.api import DEFAULT_MAX_ITER, DEFAULT_MIN_ITER, DEFAULT_RATE_FLOOR, DEFAULT_REL_TOL  # noqa: E402


def problem(B, seed=3):
    rng = np.random.default_rng(seed)
    grid = colate_amd.age_grid()
    ep, _ = colate_amd.epochs_from_bins("3,7,0.2")
    later = grid[np.minimum(np.arange(grid.size) + 3, grid.size - 1)]
    kinds = np.tile([0, 1], grid.size).astype(np.int32)
    a0, a1 = np.repeat(grid, 2), np.repeat(later, 2)
    # mean counts that fall off with age on both sides of a mode, as a genome's age spectrum does
    mean = 40.0 * np.exp(-0.5 * ((np.log(np.maximum(np.repeat(grid, 2), 1.0)) - np.log(3e3)) / 2.0) ** 2)
    w = rng.poisson(mean, (B, kinds.size)).astype(float)
    return kinds, a0, a1, w, ep


def mstep_numpy(num, den, rates, floor):
    """coal.cpp:3771-3815 (regularise == 2)"""
    with np.errstate(all="ignore"):
        own = np.where(den == 0, rates, np.maximum(num / den, floor))
    for e in range(rates.size):
        rates[e] = own[e] if num[e] != 0 else (rates[e - 1] if e > 0 else 0.0)


def host_driven_loop(kinds, a0, a1, w, ep, device):
    B, E = w.shape[0], ep.size
    out = np.zeros((B, E)), np.zeros(B, dtype=np.int32), np.zeros(B)
    for b in range(B):
        rates = np.full(E, colate_amd.api.DEFAULT_INIT_RATE)
        ll, it = -np.inf, 0
        with np.errstate(all="ignore"):
            while it < DEFAULT_MAX_ITER:
                prev = ll
                *_, nacc, dacc, ll = colate_amd.em_interval_calls(kinds, a0, a1, ep, rates, weights=w[b], device=device)
                mstep_numpy(nacc, dacc, rates, DEFAULT_RATE_FLOOR)
                if np.float64(ll) / np.float64(prev) > 1.0 - DEFAULT_REL_TOL and it > DEFAULT_MIN_ITER:
                    break
                it += 1
        out[0][b], out[1][b], out[2][b] = rates, it, ll
    return out


def timed(f, reps):
    res = f()  # warm-up: code objects, workspace, caches
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        res = f()
        walls.append(time.perf_counter() - t)
    return res, walls


def record(walls, B, iters):
    med = statistics.median(walls)
    return {"replicates": B, "iterations_total": int(np.sum(iters)), "wall_s_median": round(med, 4),
            "wall_s_all": [round(x, 4) for x in walls], "s_per_replicate": round(med / B, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "interval", "em_interval_fit_bench.json"))
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-replicates", type=int, default=5)
    ap.add_argument("--host-replicates", type=int, default=2)
    ap.add_argument("--host-only", action="store_true", help="no device runs (a machine without a GPU)")
    a = ap.parse_args()
    assert a.reps >= 3, "the median of at least 3 runs"
    kinds, a0, a1, w, ep = problem(a.replicates)
    out = {"input": f"--bins 3,7,0.2 (E = {ep.size}), R = {kinds.size}, B = {a.replicates}, max_iter {DEFAULT_MAX_ITER}, "
                    f"min_iter {DEFAULT_MIN_ITER}, rel_tol {DEFAULT_REL_TOL}", "reps": a.reps}
    nh = min(a.host_replicates, a.replicates)
    host, walls = timed(lambda: colate_amd.em_interval_batch(kinds, a0, a1, w[:nh], ep, device=False, math=1), a.reps)
    out["host_twin"] = record(walls, nh, host[1])
    print(json.dumps({"host_twin": out["host_twin"]}), flush=True)
    if a.host_only:
        out["device_call"] = out["host_driven_loop"] = "not measured (--host-only)"
    else:
        dev, walls = timed(lambda: colate_amd.em_interval_batch(kinds, a0, a1, w, ep), a.reps)
        out["device_call"] = record(walls, a.replicates, dev[1])
        out["device_call"]["iterations_min_max"] = [int(dev[1].min()), int(dev[1].max())]
        out["device_call"]["flags_or"] = int(np.bitwise_or.reduce(dev[3]))
        out["device_call"]["equals_host_twin_bits"] = bool(all(
            np.array_equal(np.ascontiguousarray(d[:nh]).view(np.uint8), np.ascontiguousarray(h).view(np.uint8)) for d, h in zip(dev, host)))
        print(json.dumps({"device_call": out["device_call"]}), flush=True)
        nl = min(a.loop_replicates, a.replicates)
        loop, walls = timed(lambda: host_driven_loop(kinds, a0, a1, w[:nl], ep, True), a.reps)
        out["host_driven_loop"] = record(walls, nl, loop[1])
        out["host_driven_loop"]["iterations_equal_device_call"] = bool(np.array_equal(loop[1], dev[1][:nl]))
        out["host_driven_loop"]["max_rel_rate_diff_vs_device_call"] = float(
            np.max(np.abs(loop[0] - dev[0][:nl]) / np.maximum(np.abs(dev[0][:nl]), 1e-300)))
        out["speedup_per_replicate"] = {
            "device_call_vs_host_driven_loop": round(out["host_driven_loop"]["s_per_replicate"] / out["device_call"]["s_per_replicate"], 1),
            "device_call_vs_host_twin": round(out["host_twin"]["s_per_replicate"] / out["device_call"]["s_per_replicate"], 1)}
    s = json.dumps(out, indent=1)
    print(s)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
