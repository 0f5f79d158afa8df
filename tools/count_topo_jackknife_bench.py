"""Measures `Colate --mode count_topo --samples --age_profile 3,7,0.2 --profile_only --jackknife` -- the counts per (triple, genome
block, epoch) formed on the device and the block jackknife on them -- against the same run without `--jackknife`, on one MI355X
(run by hand; not part of bench.py):

  * inputs: the generator and shape of tools/count_topo_bench.py -- the 20 samples of BASELINE configs[4] (22 chromosomes x 1 M
    .mut rows), 180 triples of three different lines --, or with --small 6 samples (12 triples) over small synthetic files;
  * three forms of the same binary take turns, and so does their order: (b) `--age_profile 3,7,0.2 --profile_only` on the device,
    the yardstick: the run the command line had before the option; (d) the same plus `--jackknife` (30 000 000 bases per block) on
    the device; (e) form (d) with COLATE_DEVICE_TOPO=0, the host twin of the triple stage.  One warm-up each, then the median of
    --reps (3) runs;
  * per run: wall time, and from the command line's COLATE_TIMING line the seconds of reading and indexing the inputs, of the
    triple stage, of the device's kernels alone, and of writing the files;
  * whether (d) and (e) wrote the same bytes, and whether PREFIX.profile.txt and PREFIX.triples.txt of (d) are those of (b);
  * (d) over (b), at the wall, in the triple stage and in kernel seconds.

Prints one JSON document and writes it to --record (default profiles/topo/count_topo_jackknife_bench.json, or ..._small.json)."""
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
PROFILE = ["--age_profile", BINS, "--profile_only"]
FORMS = {"profile_only_device": ("b", PROFILE, True, r"triples profiled on the device"),
         "jackknife_device": ("d", PROFILE + ["--jackknife"], True, r"triples profiled in (\d+) blocks on the device"),
         "jackknife_host_twin": ("e", PROFILE + ["--jackknife"], False, r"triples profiled in (\d+) blocks on the host")}


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
            "files_s": float(m.group(4)), "rows": int(m.group(5)), "samples": int(m.group(6)), "triples": int(m.group(7)),
            "blocks": int(s.group(1)) if s.groups() else None}


def measure(d, reps):
    names = list(FORMS)
    runs = {f: [] for f in names}
    for f in names:  # warm-up: file cache, code objects
        run(d, f)
    for k in range(reps):  # (taking turns, and the form that goes first moves on too)
        for f in names[k % 3:] + names[:k % 3]:
            runs[f].append(run(d, f))
    read = lambda name: open(os.path.join(d, name), "rb").read()  # noqa: E731
    first = runs["jackknife_device"][0]
    out = {"rows": first["rows"], "samples": first["samples"], "triples": first["triples"], "age_profile": BINS, "block_bases": 30000000,
           "blocks": first["blocks"], "jackknife_lines": read("d.jackknife.txt").count(b"\n"),
           "device_and_host_twin_equal_bytes": all(read(f"d.{n}.txt") == read(f"e.{n}.txt") for n in ("jackknife", "profile", "triples")),
           "profile_with_jackknife_equals_profile_without": read("d.profile.txt") == read("b.profile.txt") and read("d.triples.txt") == read("b.triples.txt")}
    for f in names:
        out[f] = {k + "_median": round(statistics.median(x[k] for x in runs[f]), 4) for k in ("wall_s", "inputs_s", "triple_stage_s", "kernels_s", "files_s")}
        out[f]["wall_s_all"] = [round(x["wall_s"], 3) for x in runs[f]]
        out[f]["triple_stage_s_all"] = [round(x["triple_stage_s"], 4) for x in runs[f]]
        out[f]["kernels_s_all"] = [round(x["kernels_s"], 5) for x in runs[f]]
    med = lambda f, k: out[f][k + "_median"]  # noqa: E731
    out["device_not_slower_than_host_twin"] = med("jackknife_device", "wall_s") <= med("jackknife_host_twin", "wall_s")
    out["triple_stage_device_not_slower_than_host_twin"] = med("jackknife_device", "triple_stage_s") <= med("jackknife_host_twin", "triple_stage_s")
    for k in ("wall_s", "triple_stage_s", "kernels_s"):
        out["jackknife_over_profile_only_" + k] = round(med("jackknife_device", k) / med("profile_only_device", k), 3) if med("profile_only_device", k) > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="6 samples over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.record is None:
        a.record = os.path.join(ROOT, "profiles", "topo", "count_topo_jackknife_bench_small.json" if a.small else "count_topo_jackknife_bench.json")
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="count_topo_jackknife_bench_")
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
