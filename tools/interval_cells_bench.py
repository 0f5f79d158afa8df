"""Measures colate_interval_cells (device: csrc/interval_cells_kernel.hip) against colate_interval_cells_host (the host
twin) through the C ABI, on records packed beforehand:

  * one pair's worth of records at 22 x 1 M .mut rows: 22 chromosomes of 150 Mb in 30-Mb blocks (110 genome blocks), 40 % of
    the rows used by the pair (the share tests/synth_files.py gives), ages drawn as synth_files draws them (age_begin
    10^U(1, 5.2), 8 % from age 0, age_end up to 2.5 x age_begin), weights from diploid genotypes;
  * the test size: tests/interval_cells_lib.random_records(2000, 5, 8).

Per shape and side: the first call (on the device it includes the workspace allocation), then the median of --reps calls;
whether every bit of kinds, ages, tables and the dropped count is the same on the two sides.  Prints one JSON document and
writes it to --record (default profiles/interval/interval_cells_bench.json; --host-only: ..._host.json, the host twin alone)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colate_amd  # noqa: E402
import interval_cells_lib as il  # noqa: E402
from colate_amd._lib import lib  # noqa: E402


def genome_records(chroms=22, rows_per_chr=1_000_000, used=0.4, span=150_000_000, block=30_000_000, seed=5):
    rng = np.random.default_rng(seed)
    n_chr = int(rows_per_chr * used)
    n = chroms * n_chr
    begin = (10.0 ** rng.uniform(1, 5.2, n)).astype(np.float32)
    begin[rng.uniform(size=n) < 0.08] = 0.0
    end = (np.maximum(begin, np.float32(30.0)) * (1 + 1.5 * rng.uniform(size=n))).astype(np.float32)
    daf_ref = rng.integers(1, 3, n)
    f_daf = rng.integers(0, 3, n)
    w_sh, w_ns = f_daf * daf_ref / 2.0, (2 - f_daf) * daf_ref / 2.0
    per_chr = (span + block - 1) // block
    blk = np.concatenate([c * per_chr + np.sort(rng.integers(0, span, n_chr)) // block for c in range(chroms)]).astype(np.int32)
    return begin, end, w_sh, w_ns, blk, chroms * per_chr


def pack(case):
    begin, end, w_sh, w_ns, blk, nb = case
    recs = np.zeros(begin.size, dtype=colate_amd.api.INTERVAL_REC)
    recs["begin"], recs["end"], recs["w_sh"], recs["w_ns"] = begin, end, w_sh, w_ns
    return recs, np.ascontiguousarray(blk, dtype=np.int32), int(nb)


def call(fn, recs, blk, nb):
    cap = min(colate_amd.api.INTERVAL_MAX_ROWS, 2 * recs.size)
    kinds = np.zeros(cap, dtype=np.int32)
    a0, a1, tables = np.zeros(cap), np.zeros(cap), np.zeros(nb * cap)
    dropped = ctypes.c_longlong(0)
    t = time.perf_counter()
    R = fn(recs.size, recs.ctypes.data, blk.ctypes.data, nb, cap, kinds.ctypes.data, a0.ctypes.data, a1.ctypes.data, tables.ctypes.data,
           ctypes.addressof(dropped))
    dt = time.perf_counter() - t
    if R < 0:
        raise colate_amd.ColateError(R)
    return dt, (kinds[:R].tobytes(), a0[:R].tobytes(), a1[:R].tobytes(), tables[:nb * R].tobytes(), dropped.value), R


def measure(fn, packed, reps):
    first, res, R = call(fn, *packed)  # warm-up
    times = [call(fn, *packed)[0] for _ in range(reps)]
    return {"first_call_s": round(first, 4), "median_s": round(statistics.median(times), 4), "all_s": [round(x, 4) for x in times]}, res, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-only", action="store_true", help="no device runs (a machine without a GPU)")
    a = ap.parse_args()
    if a.record is None:
        a.record = os.path.join(ROOT, "profiles", "interval", "interval_cells_bench_host.json" if a.host_only else "interval_cells_bench.json")
    out = {"reps": a.reps, "tile_cells": colate_amd.interval_cells_tile()}
    shapes = {"22 x 1M .mut rows, 40 % used": genome_records(), "test size (5 blocks x 2000 records)": il.random_records(2000, 5, 8)}
    for name, case in shapes.items():
        packed = pack(case)
        rec = {"records": int(packed[0].size), "genome_blocks": packed[2]}
        rec["host_twin"], host_res, rec["rows"] = measure(lib.colate_interval_cells_host, packed, a.reps)
        rec["dropped"] = int(host_res[4])
        if not a.host_only:
            rec["device"], dev_res, _ = measure(lib.colate_interval_cells, packed, a.reps)
            rec["device_equals_host_twin_every_bit"] = dev_res == host_res
            rec["device_not_slower_than_host_twin"] = rec["device"]["median_s"] <= rec["host_twin"]["median_s"]
        out[name] = rec
        print(json.dumps({name: rec}), flush=True)
    s = json.dumps(out, indent=1)
    print(s)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
