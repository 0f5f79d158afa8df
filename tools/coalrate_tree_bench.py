"""Measures `CoalRate --mode tree` on synthetic inputs (N = 1000 with 3000 trees and N = 5000 with 1000 trees, one
SNP-bearing span per tree; the shapes of tools/coalrate_bench.py):

  * the end-to-end CLI time on the device (one warm-up run, then the median of --reps runs), with its split into
    read+prepare / walk (COLATE_TIMING=1) and the kernel time from hip events;
  * the same with the host twin (COLATE_DEVICE_COALRATE=0), and that the two .coal files are the same bytes;
  * the reference's CoalRate once on the same input where --reference PATH names a build of it, and how many rate tokens
    of the host twin's file are identical to its.

Prints one JSON document and writes it to --record (default profiles/coalrate/coalrate_tree_bench.json)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import coalrate_lib as cl  # noqa: E402
from coalrate_bench import SHAPES, run, timing_of  # noqa: E402

ARGS = ["--mode", "tree", "-i", "in", "--bins", "3,7,0.2"]


def make_input(d, N, T, seed=11):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    with open(os.path.join(d, "in_chr1.anc"), "w") as anc, open(os.path.join(d, "in_chr1.mut"), "w") as mut:
        anc.write(f"NUM_HAPLOTYPES {N}\nNUM_TREES {T}\n")
        mut.write("snp;pos_of_snp;dist;rs-id;tree_index;branch_indices;is_not_mapping;is_flipped;age_begin;age_end;"
                  "ancestral_allele/alternative_allele;upstream_allele;downstream_allele;\n")
        for t in range(T):
            p, b = cl.random_tree(rng, N, Ne=10000.0)
            anc.write(f"{1000 + 2000 * t}: " + " ".join(f"{int(p[v])}:({b[v]:.3f} 0.000 0 0)" for v in range(2 * N - 1)) + " \n")
            mut.write(f"{t};{1000 + 2000 * t};{2000 if t + 1 < T else 1};rs{t};{t};0;0;0;10;100;A/G;A;G;\n")


def measure(d, device, reps, out_name):
    import statistics
    env = cl.cli_env(device, {"COLATE_TIMING": "1", "COLATE_DEVICE_COALRATE": "1" if device else "0"})
    cmd = [cl.CLI] + ARGS + ["-o", out_name]
    run(cmd, d, env)  # warm-up: file cache, code objects
    walls, recs = [], []
    for _ in range(reps):
        r, wall = run(cmd, d, env)
        walls.append(wall)
        recs.append(timing_of(r.stderr))
    mid = sorted(range(reps), key=lambda i: walls[i])[reps // 2]
    return {"wall_s_median": round(statistics.median(walls), 3), "wall_s_all": [round(w, 3) for w in walls], **recs[mid]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "coalrate", "coalrate_tree_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", default=None, help="a build of the reference's CoalRate to time once on the same inputs")
    ap.add_argument("--host-only", action="store_true", help="no device runs (a machine without a GPU)")
    a = ap.parse_args()
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="coalrate_tree_bench_")
    out = {"input": f"--mode tree, --bins 3,7,0.2; (N, trees) = {SHAPES}", "reps": a.reps}
    for N, T in SHAPES:
        d = os.path.join(a.workdir, f"n{N}")
        t = time.perf_counter()
        make_input(d, N, T)
        rec = {"generate_s": round(time.perf_counter() - t, 1)}
        rec["host_twin_cli"] = measure(d, False, a.reps, "host")
        if not a.host_only:
            rec["device_cli"] = measure(d, True, a.reps, "dev")
            with open(os.path.join(d, "dev.coal")) as x, open(os.path.join(d, "host.coal")) as y:
                rec["device_equals_host_twin_bytes"] = x.read() == y.read()
            rec["device_not_slower_than_host_twin"] = rec["device_cli"]["wall_s_median"] <= rec["host_twin_cli"]["wall_s_median"]
        if a.reference:
            _, wall = run([a.reference] + ARGS + ["-o", "ref"], d, dict(os.environ), timeout=3400)
            rec["reference_wall_s"] = round(wall, 2)
            total, differ = cl.compare_coal(os.path.join(d, "host.coal"), os.path.join(d, "ref.coal"))
            rec["host_twin_vs_reference_tokens"] = {"compared": total, "identical": total - differ, "not_identical": differ}
        out[f"N={N}, {T} trees"] = rec
        print(json.dumps({f"N={N}": rec}), flush=True)
    s = json.dumps(out, indent=1)
    print(s)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(s + "\n")
    if own:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
