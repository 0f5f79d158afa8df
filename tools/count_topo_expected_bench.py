"""Measures `Colate --mode count_topo --samples --age_profile 3,7,0.2 --expected --jackknife` -- the expected counts per (triple,
genome block, epoch) summed in fixed point on the device, without a draw, and the block jackknife on them -- against the sampled
run of the same shape, on one MI355X (run by hand; not part of bench.py):

  * inputs: the generator and shape of tools/count_topo_bench.py -- the 20 samples of BASELINE configs[4] (22 chromosomes x 1 M
    .mut rows), 180 triples of three different lines --, or with --small 6 samples (12 triples) over small synthetic files;
  * three forms of the same binary take turns, and so does their order: (d) `--age_profile 3,7,0.2 --profile_only --jackknife` on
    the device, the yardstick: the sampled counts per block and their jackknife; (x) `--age_profile 3,7,0.2 --expected --jackknife`
    on the device; (y) form (x) with COLATE_DEVICE_TOPO=0, the host twin of the triple stage.  One warm-up each, then the median of
    --reps (3) runs;
  * per run: wall time, and from the command line's COLATE_TIMING line the seconds of reading and indexing the inputs (for (d) these
    hold the run's stream of uniforms, which (x) does not form), of the triple stage, of the device's kernels alone, and of writing
    the files;
  * whether (x) and (y) wrote the same bytes;
  * expected_not_slower_than_sampled: the median wall of (x) against that of (d) plus the spread (max - min) of (d)'s runs;
    device_not_slower_than_host_twin: (x) against (y); both recorded whichever way they fall; (x) over (d) at the wall, in the inputs,
    in the triple stage and in kernel seconds.

Prints one JSON document and writes it to --record (default profiles/topo/count_topo_expected_bench.json, or ..._small.json)."""
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
BINS = "3,7,0.2"
FORMS = {"sampled_jackknife_device": ("d", ["--age_profile", BINS, "--profile_only", "--jackknife"], True, r"triples profiled in (\d+) blocks on the device"),
         "expected_jackknife_device": ("x", ["--age_profile", BINS, "--expected", "--jackknife"], True, r"triples expected in (\d+) blocks on the device"),
         "expected_jackknife_host_twin": ("y", ["--age_profile", BINS, "--expected", "--jackknife"], False, r"triples expected in (\d+) blocks on the host")}
KEYS = ("wall_s", "inputs_s", "triple_stage_s", "kernels_s", "files_s")


def run(d, form):
    out, more, device, said = FORMS[form]
    env = dict(os.environ, COLATE_TIMING="1")
    for k in ("COLATE_DEVICE_TOPO", "COLATE_INDEXED_WALK", "COLATE_TOPO_BUDGET"):
        env.pop(k, None)
    if not device:
        env["COLATE_DEVICE_TOPO"] = "0"
    t = time.perf_counter()
    r = subprocess.run([pb.CLI, "--mode", "count_topo", "--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", "5", "-o", out] + more,
                       cwd=d, capture_output=True, text=True, env=env, timeout=3400)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    s = re.search(said, r.stderr)
    assert s, r.stderr[-1500:]
    assert device == ("on the host" not in r.stderr), "no device: this measurement needs one\n" + r.stderr[-1500:]
    m = re.search("Timing: count_topo samples: inputs " + NUM + " s, triple stage " + NUM + r" s \(device kernels " + NUM + r" s\), files " + NUM
                  + r" s; (\d+) rows, (\d+) samples, (\d+) triples", r.stderr)
    assert m, r.stderr[-1500:]
    print(f"{form}: {wall:.2f} s", file=sys.stderr, flush=True)  # (a line per run, so that a long measurement shows where it is)
    return {"wall_s": wall, "inputs_s": float(m.group(1)), "triple_stage_s": float(m.group(2)), "kernels_s": float(m.group(3)),
            "files_s": float(m.group(4)), "rows": int(m.group(5)), "samples": int(m.group(6)), "triples": int(m.group(7)), "blocks": int(s.group(1))}


def measure(d, reps):
    names = list(FORMS)
    runs = {f: [] for f in names}
    for f in names:  # warm-up: file cache, code objects
        run(d, f)
    for k in range(reps):  # (taking turns, and the form that goes first moves on too)
        for f in names[k % 3:] + names[:k % 3]:
            runs[f].append(run(d, f))
    read = lambda name: open(os.path.join(d, name), "rb").read()  # noqa: E731
    first = runs["expected_jackknife_device"][0]
    out = {"rows": first["rows"], "samples": first["samples"], "triples": first["triples"], "age_profile": BINS, "block_bases": 30000000,
           "blocks": first["blocks"], "expected_lines": read("x.expected.txt").count(b"\n"),
           "expected_jackknife_lines": read("x.expected.jackknife.txt").count(b"\n"),
           "device_and_host_twin_equal_bytes": all(read(f"x.{n}.txt") == read(f"y.{n}.txt") for n in ("expected", "expected.jackknife"))}
    for f in names:
        out[f] = {k + "_median": round(statistics.median(x[k] for x in runs[f]), 4) for k in KEYS}
        for k in ("wall_s", "inputs_s", "triple_stage_s", "kernels_s"):
            out[f][k + "_all"] = [round(x[k], 5) for x in runs[f]]
    med = lambda f, k: out[f][k + "_median"]  # noqa: E731
    walls = [x["wall_s"] for x in runs["sampled_jackknife_device"]]
    out["sampled_wall_spread_s"] = round(max(walls) - min(walls), 4)
    out["expected_not_slower_than_sampled"] = med("expected_jackknife_device", "wall_s") <= med("sampled_jackknife_device", "wall_s") + (max(walls) - min(walls))
    out["device_not_slower_than_host_twin"] = med("expected_jackknife_device", "wall_s") <= med("expected_jackknife_host_twin", "wall_s")
    out["triple_stage_device_not_slower_than_host_twin"] = med("expected_jackknife_device", "triple_stage_s") <= med("expected_jackknife_host_twin", "triple_stage_s")
    for k in ("wall_s", "inputs_s", "triple_stage_s", "kernels_s"):
        base = med("sampled_jackknife_device", k)
        out["expected_over_sampled_" + k] = round(med("expected_jackknife_device", k) / base, 3) if base > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="6 samples over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.record is None:
        a.record = os.path.join(ROOT, "profiles", "topo", "count_topo_expected_bench_small.json" if a.small else "count_topo_expected_bench.json")
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="count_topo_expected_bench_")
    os.makedirs(a.workdir, exist_ok=True)
    pairs = pb.make_inputs(a.workdir, a.small)
    targets, refs = sorted({t for t, _, _ in pairs}), sorted({r for _, r, _ in pairs})
    files = targets + refs
    with open(os.path.join(a.workdir, "samples.txt"), "w") as f:
        for k, fn in enumerate(targets):
            f.write(f"{fn.split('.')[0]} {fn} role={'cond,target' if k < 2 else 'target'}\n")
        for fn in refs:
            f.write(f"{fn.split('.')[0]} {fn} role=reference\n")
    out = {"input": (f"{len(files)} samples, 2 chromosomes x 1500 .mut rows" if a.small
                     else f"{len(files)} samples, 22 chromosomes x 1 M .mut rows (BASELINE configs[4])")
           + f"; 2 cond x {len(targets)} targets x {len(refs)} references, three different lines each", "reps": a.reps}
    out.update(measure(a.workdir, a.reps))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.record), exist_ok=True)
    with open(a.record, "w") as f:
        f.write(text + "\n")
    if own:
        shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
