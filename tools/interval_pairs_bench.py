"""Measures `Colate --mode mut_interval --pairs` against the single-pair runs it replaces, on one MI355X (run by hand; not
part of bench.py):

  * inputs: the 10 x 10 pairs of BASELINE configs[4]'s inputs (22 chromosomes x 1 M .mut rows, tools/gen_wg_inputs.cpp), or
    with --small 3 x 3 pairs over the synthetic files of tests/synth_files.py;
  * B = 20 bootstrap replicates, --bins 3,7,0.2, --seed 3; one warm-up, then the median of --reps (3) runs;
  * `--pairs LIST` in one process against the SUM of the single runs `--mut P --target_tmp T --reference_tmp R -o OUT` of
    the same binary, one process per pair (that path is the baseline);
  * the seconds the kernels of the --pairs run took on the device (its COLATE_TIMING line), and whether every OUT.coal of
    the --pairs run is, byte for byte, the file of its single run.

Prints one JSON document and writes it to --record (default profiles/interval/interval_pairs_bench.json) with both times, the
kernel seconds and `pairs_not_slower_than_single_runs`."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")
FIT = ["--bins", "3,7,0.2", "--num_bootstraps", "20", "--seed", "3"]


def make_inputs(d, small):
    """the files and the list of (target, reference, output) names, relative to d"""
    if small:
        import synth_files
        synth_files.write_inputs(d, chroms=("1", "2"), snps_per_chr=1500, extra_targets=2, extra_refs=2)
        n = 3
    else:
        gen = os.path.join(d, "gen")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "gen_wg_inputs.cpp"), "-lz", "-o", gen])
        subprocess.check_call([gen, d, "22", "1000000", "plain", "10", "10"], stdout=subprocess.DEVNULL)
        n = 10
    name = lambda s, i: f"{s}{i if i else ''}.colate.in"  # noqa: E731
    return [(name("T", i), name("R", j), f"{i}_{j}") for i in range(n) for j in range(n)]


def run(args, d, timeout=3400):
    env = dict(os.environ, COLATE_TIMING="1")
    env.pop("COLATE_DEVICE_INTERVAL", None)
    t = time.perf_counter()
    r = subprocess.run([CLI, "--mode", "mut_interval", "--mut", "P", "--chr", "chr.txt"] + FIT + args, cwd=d, capture_output=True, text=True,
                       env=env, timeout=timeout)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    assert "on the host" not in r.stderr, "no device: this measurement needs one"
    return r, wall


def pairs_run(d, pairs):
    with open(os.path.join(d, "list.txt"), "w") as f:
        for t, r, out in pairs:
            f.write(f"{t} {r} pairs_{out}\n")
    r, wall = run(["--pairs", "list.txt"], d)
    m = re.search(r"Timing: interval pairs: inputs and walks ([\d.e+-]+) s, cells, rows and fits ([\d.e+-]+) s \(device kernels ([\d.e+-]+) s\)", r.stderr)
    assert m, r.stderr[-1500:]
    return {"wall_s": wall, "inputs_and_walks_s": float(m.group(1)), "cells_rows_fits_s": float(m.group(2)), "kernels_s": float(m.group(3))}


def single_runs(d, pairs):
    return sum(run(["--target_tmp", t, "--reference_tmp", r, "-o", f"single_{out}"], d)[1] for t, r, out in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="3 x 3 pairs over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "interval", "interval_pairs_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="interval_pairs_bench_")
    os.makedirs(a.workdir, exist_ok=True)
    pairs = make_inputs(a.workdir, a.small)
    def timed(what, fn):  # (a line per run, so that a long measurement shows where it is)
        t = time.perf_counter()
        r = fn(a.workdir, pairs)
        print(f"{what}: {time.perf_counter() - t:.2f} s", file=sys.stderr, flush=True)
        return r

    timed("warm-up, --pairs", pairs_run), timed("warm-up, single runs", single_runs)  # file cache, code objects
    p = [timed("--pairs", pairs_run) for _ in range(a.reps)]
    s = [timed("single runs", single_runs) for _ in range(a.reps)]
    mid = sorted(p, key=lambda x: x["wall_s"])[a.reps // 2]
    same = all(open(os.path.join(a.workdir, f"pairs_{o}.coal"), "rb").read() == open(os.path.join(a.workdir, f"single_{o}.coal"), "rb").read()
               for _, _, o in pairs)
    out = {"input": ("3 x 3 pairs, 2 chromosomes x 1500 .mut rows" if a.small else "10 x 10 pairs, 22 chromosomes x 1 M .mut rows (BASELINE configs[4])")
           + "; B = 20, --bins 3,7,0.2, --seed 3", "pairs": len(pairs), "reps": a.reps,
           "pairs_wall_s_median": round(statistics.median(x["wall_s"] for x in p), 3), "pairs_wall_s_all": [round(x["wall_s"], 3) for x in p],
           "pairs_inputs_and_walks_s": mid["inputs_and_walks_s"], "pairs_cells_rows_fits_s": mid["cells_rows_fits_s"],
           "pairs_kernels_s": mid["kernels_s"],
           "single_runs_wall_s_median": round(statistics.median(s), 3), "single_runs_wall_s_all": [round(x, 3) for x in s],
           "coal_files_equal_bytes": same}
    out["pairs_not_slower_than_single_runs"] = out["pairs_wall_s_median"] <= out["single_runs_wall_s_median"]
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(text + "\n")
    if own:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
