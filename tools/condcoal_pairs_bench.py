"""Measures `Colate --mode CondCoalRates --pairs` on tools/condcoal_bench.py's input (N = 500 haplotypes, 5000 trees, ten
groups of 50), modern and ancient, over all 100 ordered group pairs:

  * the wall time of one --pairs run on the device, split into parse / walk / bootstrap+write and kernel time
    (COLATE_TIMING=1);
  * the sum of the wall times of the 100 single runs (`--groups FOCAL,COND`) on the device, and that every --pairs table is
    byte-identical to its single run;
  * the reference's `Colate` (oracle/_ref/Colate_ref, where it was built) on the first --ref-pairs pairs, extrapolated to 100;
  * with --rocprof, one `rocprofv3 --kernel-trace --stats` run of the --pairs CLI (every kernel's calls and time).

Prints one JSON document (and writes it to --record)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import condcoal_bench as cb  # noqa: E402


def kernel_stats(path):
    """{kernel: calls / total / average} of the condcoal kernels in a rocprofv3 kernel_stats.csv."""
    kern = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"(condcoal\w*)\(", row.get("Name", ""))
            if m:
                kern[m.group(1)] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3),
                                    "avg_ms": round(float(row["AverageNs"]) / 1e6, 3)}
    return kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=None, help="where the inputs are written (default: a new temporary directory)")
    ap.add_argument("--record", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--ref-pairs", type=int, default=10, help="pairs of the reference loop (0: none)")
    ap.add_argument("--variants", default="modern,ancient")
    a = ap.parse_args()
    own_workdir = a.workdir is None
    if own_workdir:
        a.workdir = tempfile.mkdtemp(prefix="condcoal_pairs_bench_")
    out = {"input": "N=500, 5000 trees, ten groups of 50 haplotypes, all 100 ordered pairs, default epochs, --lineage_bin 4"}
    for variant in a.variants.split(","):
        d = os.path.join(a.workdir, variant)
        t = time.perf_counter()
        cb.make_input(d, variant == "ancient")
        rec = {"generate_s": round(time.perf_counter() - t, 2)}
        with open(os.path.join(d, "in.poplabels")) as f:
            groups = sorted({line.split()[1] for line in f.read().splitlines()[1:] if line.strip()})
        pairs = [f"{x},{y}" for x in groups for y in groups]
        with open(os.path.join(d, "list.txt"), "w") as f:
            f.write("".join(f"{g} p{k}.txt\n" for k, g in enumerate(pairs)))
        shared = ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels", "--lineage_bin", "4", "--seed", "1"]
        env = dict(os.environ, COLATE_TIMING="1")
        r, wall = cb.run([cb.CLI] + shared + ["--pairs", "list.txt"], d, env)
        assert r.returncode == 0, r.stderr[-2000:]
        rec["pairs"] = len(pairs)
        rec["pairs_cli"] = {"wall_s": round(wall, 3), **(cb.timing_of(r.stderr) or {})}
        solo, kern, same = 0.0, 0.0, 0
        for k, g in enumerate(pairs):
            r, wall = cb.run([cb.CLI] + shared + ["--groups", g, "-o", f"s{k}.txt"], d, env)
            assert r.returncode == 0, (g, r.stderr[-2000:])
            solo += wall
            kern += (cb.timing_of(r.stderr) or {}).get("kernels_s", 0.0)
            with open(os.path.join(d, f"p{k}.txt"), "rb") as f1, open(os.path.join(d, f"s{k}.txt"), "rb") as f2:
                same += f1.read() == f2.read()
        rec["solo_loop"] = {"wall_s_sum": round(solo, 3), "kernels_s_sum": round(kern, 3)}
        rec["pairs_tables_identical_to_solo"] = f"{same}/{len(pairs)}"
        rec["solo_over_pairs_wall"] = round(solo / rec["pairs_cli"]["wall_s"], 1)
        if a.ref_pairs and os.path.exists(cb.REF):
            t_ref, worst = 0.0, 0.0
            for k, g in enumerate(pairs[:a.ref_pairs]):
                r, wall = cb.run([cb.REF] + shared + ["--groups", g, "--output", f"ref{k}.txt"], d, timeout=1200)
                assert r.returncode == 0, (g, r.stderr[-2000:])
                t_ref += wall
                worst = max(worst, cb.cl.compare_tables(os.path.join(d, f"p{k}.txt"), os.path.join(d, f"ref{k}.txt"), 1.0))
            rec["reference_loop"] = {"pairs_run": a.ref_pairs, "wall_s": round(t_ref, 2),
                                     "extrapolated_100_pairs_s": round(t_ref * len(pairs) / a.ref_pairs, 1),
                                     "pairs_vs_reference_max_rel": worst}
        if a.rocprof and shutil.which("rocprofv3"):
            pdir = os.path.join(d, "rocprof")
            shutil.rmtree(pdir, ignore_errors=True)
            r, _ = cb.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "ccp", "--",
                           cb.CLI] + shared + ["--pairs", "list.txt"], d)
            kern = {}
            for path in glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True):
                kern.update(kernel_stats(path))
            rec["rocprofv3_kernels"] = kern or f"no stats (rc={r.returncode})"
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
