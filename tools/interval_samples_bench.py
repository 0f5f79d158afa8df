"""Measures `Colate --mode mut_interval --samples` against `--pairs` on the expanded list, same binary, on one MI355X (run by
hand; not part of bench.py):

  * inputs: those of tools/interval_pairs_bench.py -- 10 targets x 10 references over BASELINE configs[4]'s inputs (22
    chromosomes x 1 M .mut rows), or with --small 3 x 3 over the synthetic files of tests/synth_files.py; B = 20,
    --bins 3,7,0.2, --seed 3;
  * the two forms alternate, and so does the one that goes first; one warm-up each, then the median of --reps (3) runs;
  * once at the default iteration limits (the fit dominates) and once with --max_iter 2 --min_iter 1 (the front end shows);
  * per run: wall time, the seconds the kernels took on the device (the COLATE_TIMING line; for --samples with both walk
    passes), the bytes copied host to device as counted from shapes (--pairs: 24 bytes per record; --samples: 12 bytes per
    row, 8 bytes per row and sample, the masks' words), and the process's peak memory (the footer of the command line);
  * whether every .coal of --samples is, byte for byte, the file of --pairs.

Prints one JSON document and writes it to --record (default profiles/interval/interval_samples_bench.json)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import interval_pairs_bench as pb  # noqa: E402

NUM = r"([\d.e+-]+)"


def run(args, d, limits):
    env = dict(os.environ, COLATE_TIMING="1")
    for k in ("COLATE_DEVICE_INTERVAL", "COLATE_DEVICE_INTERVAL_WALK"):
        env.pop(k, None)
    t = time.perf_counter()
    r = subprocess.run([pb.CLI, "--mode", "mut_interval", "--mut", "P", "--chr", "chr.txt"] + pb.FIT + limits + args, cwd=d,
                       capture_output=True, text=True, env=env, timeout=3400)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    assert "on the host" not in r.stderr, "no device: this measurement needs one"
    rss = re.search(r"Max Memory usage: " + NUM + "Mb", r.stderr)
    return r.stderr, {"wall_s": wall, "peak_rss_mb": float(rss.group(1)) if rss else None}


def pairs_run(d, limits):
    err, out = run(["--pairs", "list.txt"], d, limits)
    m = re.search(r"\(device kernels " + NUM + r" s\); (\d+) records uploaded", err)
    assert m, err[-1500:]
    out.update(kernels_s=float(m.group(1)), h2d_bytes=24 * int(m.group(2)))
    return out


def samples_run(d, limits):
    err, out = run(["--samples", "samples.txt", "-o", "samples"], d, limits)
    m = re.search(r"\(device kernels " + NUM + r" s\); (\d+) rows, (\d+) index arrays and (\d+) masks staged, (\d+) records formed", err)
    assert m and "walked on the device" in err, err[-1500:]
    rows, S, M = int(m.group(2)), int(m.group(3)), int(m.group(4))
    out.update(kernels_s=float(m.group(1)), h2d_bytes=12 * rows + 8 * S * rows + M * (rows // 8 + 8), records_formed=int(m.group(5)))
    return out


def median_of(runs, key):
    v = [x[key] for x in runs if x[key] is not None]
    return round(statistics.median(v), 3) if v else None


def measure(d, pairs, limits, reps):
    def timed(what, fn):  # (a line per run, so that a long measurement shows where it is)
        t = time.perf_counter()
        r = fn(d, limits)
        print(f"{what} {' '.join(limits)}: {time.perf_counter() - t:.2f} s", file=sys.stderr, flush=True)
        return r

    timed("warm-up, --samples", samples_run), timed("warm-up, --pairs", pairs_run)  # file cache, code objects
    s, p = [], []
    for k in range(reps):  # (alternating, and the form that goes first alternates too)
        for form in (("s", "p") if k % 2 == 0 else ("p", "s")):
            if form == "s":
                s.append(timed("--samples", samples_run))
            else:
                p.append(timed("--pairs", pairs_run))
    same = all(open(os.path.join(d, f"samples_t{o.split('_')[0]}_r{o.split('_')[1]}.coal"), "rb").read()
               == open(os.path.join(d, f"pairs_{o}.coal"), "rb").read() for _, _, o in pairs)
    out = {"limits": " ".join(limits) or "default (--max_iter 100000 --min_iter 1000)", "coal_files_equal_bytes": same}
    for name, runs in (("samples", s), ("pairs", p)):
        out[name] = {"wall_s_median": median_of(runs, "wall_s"), "wall_s_all": [round(x["wall_s"], 3) for x in runs],
                     "kernels_s_median": median_of(runs, "kernels_s"), "kernels_s_all": [round(x["kernels_s"], 3) for x in runs], "h2d_bytes": runs[0]["h2d_bytes"],
                     "peak_rss_mb_median": median_of(runs, "peak_rss_mb")}
    out["samples"]["records_formed"] = s[0]["records_formed"]
    out["samples_not_slower_than_pairs"] = out["samples"]["wall_s_median"] <= out["pairs"]["wall_s_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="3 x 3 pairs over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "interval", "interval_samples_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="interval_samples_bench_")
    os.makedirs(a.workdir, exist_ok=True)
    pairs = pb.make_inputs(a.workdir, a.small)
    with open(os.path.join(a.workdir, "list.txt"), "w") as f:
        for t, r, out in pairs:
            f.write(f"{t} {r} pairs_{out}\n")
    n = round(len(pairs) ** 0.5)
    name = lambda s, i: f"{s}{i if i else ''}.colate.in"  # noqa: E731
    with open(os.path.join(a.workdir, "samples.txt"), "w") as f:
        for i in range(n):
            f.write(f"t{i} {name('T', i)} role=target\n")
        for j in range(n):
            f.write(f"r{j} {name('R', j)} role=reference\n")
    out = {"input": ("3 x 3 pairs, 2 chromosomes x 1500 .mut rows" if a.small else "10 x 10 pairs, 22 chromosomes x 1 M .mut rows (BASELINE configs[4])")
           + "; B = 20, --bins 3,7,0.2, --seed 3", "pairs": len(pairs), "reps": a.reps,
           "runs": [measure(a.workdir, pairs, [], a.reps), measure(a.workdir, pairs, ["--max_iter", "2", "--min_iter", "1"], a.reps)]}
    out["samples_not_slower_than_pairs"] = all(r["samples_not_slower_than_pairs"] for r in out["runs"])
    out["coal_files_equal_bytes"] = all(r["coal_files_equal_bytes"] for r in out["runs"])
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(text + "\n")
    if own:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
