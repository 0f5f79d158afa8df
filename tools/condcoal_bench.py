"""Measures `Colate --mode CondCoalRates` on a synthetic input (N = 500 haplotypes, 5000 trees, ten groups of 50: focal and
conditional groups of 50 each), modern and ancient:

  * the end-to-end CLI time on the device, split into parse / walk / bootstrap+write (COLATE_TIMING=1), and the kernel time
    from hip events;
  * the same with the host twin (COLATE_DEVICE_CONDCOAL=0);
  * the reference's `Colate` (oracle/_ref/Colate_ref, where it was built) once on the same input, and the rate comparison;
  * with --rocprof, one `rocprofv3 --kernel-trace --stats` run of the device CLI.

Prints one JSON document (and writes it to --record)."""
import argparse
import csv
import glob
import json
import os
import random
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import condcoal_lib as cl  # noqa: E402
import condcoal_synth as cs  # noqa: E402

CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")
REF = os.path.join(ROOT, "oracle", "_ref", "Colate_ref")


def make_input(d, ancient, N=500, T=5000, seed=5):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    rnd = random.Random(seed)
    ages = cs.ancient_ages(rng, N) if ancient else None
    offset = float(ages.max()) if ancient else 0.0

    def tree(n, _ages):
        p, h = cl.random_tree(rnd, n, age_offset=offset)
        h = np.round(h, 2)
        if _ages is not None:
            h[:n] = _ages
        return p, h

    cs.write_poplabels(os.path.join(d, "in.poplabels"), N, 10, rng)
    cs.write_chromosome(os.path.join(d, "in"), rng, N, T, ages, span=120_000_000, tree_fn=tree)
    # ten groups over 250 diploid samples: make every group exactly 50 haplotypes (25 samples each)
    with open(os.path.join(d, "in.poplabels")) as f:
        rows = f.read().splitlines()
    names = sorted({r.split()[1] for r in rows[1:]})
    with open(os.path.join(d, "in.poplabels"), "w") as f:
        f.write(rows[0] + "\n")
        for i, r in enumerate(rows[1:]):
            c = r.split()
            c[1] = names[i % 10]
            f.write(" ".join(c) + "\n")


def run(cmd, cwd, env=None, timeout=900):
    t = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=env, timeout=timeout)
    return r, time.perf_counter() - t


def timing_of(stderr):
    m = re.search(r"condcoal timing: parse ([\d.]+) s, walk ([\d.]+) s \((device kernels|host twin) ([\d.]+) s\), "
                  r"bootstrap\+write ([\d.]+) s, total ([\d.]+) s", stderr)
    if not m:
        return None
    return {"parse_s": float(m.group(1)), "walk_wait_s": float(m.group(2)), "kernels_s": float(m.group(4)),
            "bootstrap_write_s": float(m.group(5)), "total_s": float(m.group(6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=None, help="where the inputs are written (default: a new temporary directory)")
    ap.add_argument("--record", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    own_workdir = a.workdir is None
    if own_workdir:
        a.workdir = tempfile.mkdtemp(prefix="condcoal_bench_")
    out = {"input": "N=500, 5000 trees, focal / conditional groups of 50 haplotypes (groups PA,PB of ten), default epochs, "
                    "--lineage_bin 4"}
    for variant in ("modern", "ancient"):
        d = os.path.join(a.workdir, variant)
        t = time.perf_counter()
        make_input(d, variant == "ancient")
        rec = {"generate_s": round(time.perf_counter() - t, 2)}
        args = ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels", "--groups", "PA,PB",
                "--lineage_bin", "4", "--seed", "1"]
        env = dict(os.environ, COLATE_TIMING="1")
        r, wall = run([CLI] + args + ["-o", "dev.txt"], d, env)
        assert r.returncode == 0, r.stderr[-2000:]
        rec["device_cli"] = {"wall_s": round(wall, 3), **(timing_of(r.stderr) or {})}
        env_h = dict(env, COLATE_DEVICE_CONDCOAL="0")
        r, wall = run([CLI] + args + ["-o", "host.txt"], d, env_h)
        assert r.returncode == 0, r.stderr[-2000:]
        rec["host_twin_cli"] = {"wall_s": round(wall, 3), **(timing_of(r.stderr) or {})}
        rec["device_vs_host_twin_max_rel"] = cl.compare_tables(os.path.join(d, "dev.txt"), os.path.join(d, "host.txt"), 1e-6)
        if not a.no_ref and os.path.exists(REF):
            r, wall = run([REF] + args + ["--output", "ref.txt"], d, timeout=1200)
            rec["reference_wall_s"] = round(wall, 2) if r.returncode == 0 else f"failed rc={r.returncode}"
            if r.returncode == 0:
                try:
                    rec["device_vs_reference_max_rel"] = cl.compare_tables(os.path.join(d, "dev.txt"), os.path.join(d, "ref.txt"), 1.0)
                except AssertionError as e:
                    rec["device_vs_reference"] = f"token mismatch: {e}"
        if a.rocprof and shutil.which("rocprofv3"):
            pdir = os.path.join(d, "rocprof")
            shutil.rmtree(pdir, ignore_errors=True)
            r, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "cc", "--", CLI] + args + ["-o", "prof.txt"], d)
            kern = {}
            for path in glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if "condcoal" in row.get("Name", ""):
                            kern = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6,
                                    "avg_ms": float(row["AverageNs"]) / 1e6}
            rec["rocprofv3_condcoal_kernel"] = kern or f"no stats (rc={r.returncode})"
        out[variant] = rec
    s = json.dumps(out, indent=1)
    print(s)
    if a.record:
        with open(a.record, "w") as f:
            f.write(s + "\n")
    if own_workdir:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
