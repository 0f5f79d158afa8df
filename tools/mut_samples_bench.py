"""Measures `Colate --mode mut --samples` against `--mode mut --pairs` on the expanded list, same binary, on one MI355X (run by
hand; not part of bench.py):

  * inputs: those of tools/interval_pairs_bench.py -- 10 targets x 10 references over BASELINE configs[4]'s inputs (22
    chromosomes x 1 M .mut rows), or with --small 3 x 3 over the synthetic files of tests/synth_files.py; B = 20,
    --bins 3,7,0.2, --seed 3;
  * the two forms alternate, and so does the one that goes first; one warm-up each, then the median of --reps (3) runs;
  * per run: wall time; the seconds the device reports -- for --samples the events around the kernels of the fill (walk
    passes, row-0 sums, jobs, age sampling), for --pairs the engine's "copies and kernels" of its age-sampling launches,
    which include its record copies: the two are reported as what they are, not as like for like --; the bytes copied host to
    device as counted from shapes (--pairs: 24 bytes per used SNP and 8 per uniform of the stream; --samples: 12 bytes per
    row, 8 per row and sample, the masks' words, and 8 per uniform of the one stream); and the process's peak memory (the
    footer of the command line);
  * whether every .coal of --samples is, byte for byte, the file of --pairs.

Prints one JSON document and writes it to --record (default profiles/mut/mut_samples_bench.json, or ..._small.json)."""
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


def run(args, d):
    env = dict(os.environ, COLATE_TIMING="1")
    for k in ("COLATE_DEVICE_FILL", "COLATE_DEVICE_FILL_WALK", "COLATE_INDEXED_WALK", "COLATE_FILL_SAMPLES_RECS_MB"):
        env.pop(k, None)
    t = time.perf_counter()
    r = subprocess.run([pb.CLI, "--mode", "mut", "--mut", "P", "--chr", "chr.txt"] + pb.FIT + args, cwd=d, capture_output=True, text=True,
                       env=env, timeout=3400)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    rss = re.search(r"Max Memory usage: " + NUM + "Mb", r.stderr)
    fill = re.search(r"pairs' table fill " + NUM + " s", r.stderr)
    return r.stderr, {"wall_s": wall, "peak_rss_mb": float(rss.group(1)) if rss else None, "table_fill_s": float(fill.group(1)) if fill else None}


def pairs_run(d):
    err, out = run(["--pairs", "list.txt"], d)
    m = re.search(r"\((\d+) used SNPs, .*age sampling on the GPU: \d+ \(pair, block\) jobs, (\d+) SNPs in \d+ launches, " + NUM + " s of copies and kernels", err)
    assert m, "no device fill in the --pairs run: this measurement needs one\n" + err[-1500:]
    out.update(device_s=float(m.group(3)), used_snps=int(m.group(1)), h2d_bytes=None)
    return out


def samples_run(d):
    err, out = run(["--samples", "samples.txt", "-o", "samples"], d)
    m = re.search(r"\(device kernels " + NUM + r" s, (\d+) chunk\(s\)\); (\d+) rows, (\d+) index arrays and (\d+) masks staged, (\d+) uniforms uploaded", err)
    assert m and "walked and filled on the device" in err, err[-1500:]
    hb = re.search(r"\((\d+) handed back to the host\)", err)
    rows, S, M = int(m.group(3)), int(m.group(4)), int(m.group(5))
    out.update(device_s=float(m.group(1)), chunks=int(m.group(2)), handed_back=int(hb.group(1)), staged_bytes=12 * rows + 8 * S * rows + M * (rows // 8 + 8), stream_bytes=8 * int(m.group(6)))
    return out


def median_of(runs, key):
    v = [x[key] for x in runs if x.get(key) is not None]
    return round(statistics.median(v), 3) if v else None


def measure(d, pairs, reps):
    def timed(what, fn):  # (a line per run, so that a long measurement shows where it is)
        t = time.perf_counter()
        r = fn(d)
        print(f"{what}: {time.perf_counter() - t:.2f} s", file=sys.stderr, flush=True)
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
    # bytes host to device, from shapes: every pair of --pairs ships its used SNPs as 24-byte records; both forms ship the seed's
    # uniforms once, 100 per used SNP of the pair that uses most (the engine's windows round that up: not counted)
    used, stream_bytes = p[0]["used_snps"], s[0]["stream_bytes"]
    out = {"coal_files_equal_bytes": same}
    for name, runs in (("samples", s), ("pairs", p)):
        out[name] = {"wall_s_median": median_of(runs, "wall_s"), "wall_s_all": [round(x["wall_s"], 3) for x in runs],
                     "table_fill_s_median": median_of(runs, "table_fill_s"), "device_s_median": median_of(runs, "device_s"),
                     "device_s_all": [round(x["device_s"], 3) for x in runs], "peak_rss_mb_median": median_of(runs, "peak_rss_mb")}
    out["pairs"]["device_s_is"] = "copies and kernels of the age-sampling launches"
    out["samples"]["device_s_is"] = "kernels of the fill: walk passes, row-0 sums, jobs, age sampling"
    out["pairs"]["h2d_bytes_from_shapes"] = 24 * used + stream_bytes
    out["samples"]["h2d_bytes_from_shapes"] = s[0]["staged_bytes"] + stream_bytes
    out["samples"]["chunks"], out["samples"]["handed_back"] = s[0]["chunks"], s[0]["handed_back"]
    out["used_snps_all_pairs"] = used
    out["samples_not_slower_than_pairs"] = out["samples"]["wall_s_median"] <= out["pairs"]["wall_s_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="3 x 3 pairs over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.record is None:
        a.record = os.path.join(ROOT, "profiles", "mut", "mut_samples_bench_small.json" if a.small else "mut_samples_bench.json")
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="mut_samples_bench_")
    os.makedirs(a.workdir, exist_ok=True)
    pairs = pb.make_inputs(a.workdir, a.small)
    with open(os.path.join(a.workdir, "list.txt"), "w") as f:
        for t, r, out in pairs:
            f.write(f"{t} {r} pairs_{out} 0 0\n")
    n = round(len(pairs) ** 0.5)
    name = lambda s, i: f"{s}{i if i else ''}.colate.in"  # noqa: E731
    with open(os.path.join(a.workdir, "samples.txt"), "w") as f:
        for i in range(n):
            f.write(f"t{i} {name('T', i)} role=target\n")
        for j in range(n):
            f.write(f"r{j} {name('R', j)} role=reference\n")
    out = {"input": ("3 x 3 pairs, 2 chromosomes x 1500 .mut rows" if a.small else "10 x 10 pairs, 22 chromosomes x 1 M .mut rows (BASELINE configs[4])")
           + "; B = 20, --bins 3,7,0.2, --seed 3", "n_pairs": len(pairs), "reps": a.reps}
    out.update(measure(a.workdir, pairs, a.reps))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(text + "\n")
    if own:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
