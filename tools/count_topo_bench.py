"""Measures `Colate --mode count_topo --samples` on the device against the same binary with COLATE_DEVICE_TOPO=0 (the host twin
of the triple stage), on one MI355X (run by hand; not part of bench.py):

  * inputs: those of tools/interval_pairs_bench.py -- the 20 samples of BASELINE configs[4] (22 chromosomes x 1 M .mut rows):
    10 targets, of which the first two are the cond samples as well, and 10 references: 2 x 9 x 10 = 180 triples of three
    different lines --, or with --small 6 samples (2 x 2 x 3 = 12 triples) over the synthetic files of tests/synth_files.py;
  * the two forms take turns, and so does the one that goes first; one warm-up each, then the median of --reps (3) runs;
  * per run: wall time, and from the command line's COLATE_TIMING line the seconds of reading and indexing the inputs, of the
    triple stage (the seed's stream, planes, counts and draws, with the upload and the waits on the device, and the lines from
    the set bits), of the device's kernels alone, and of writing the files;
  * whether every file of the device run is, byte for byte, the host twin's.

Prints one JSON document and writes it to --record (default profiles/topo/count_topo_bench.json, or ..._small.json)."""
import argparse
import glob
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


def run(d, out, device):
    env = dict(os.environ, COLATE_TIMING="1")
    for k in ("COLATE_DEVICE_TOPO", "COLATE_INDEXED_WALK", "COLATE_TOPO_BUDGET"):
        env.pop(k, None)
    if not device:
        env["COLATE_DEVICE_TOPO"] = "0"
    t = time.perf_counter()
    r = subprocess.run([pb.CLI, "--mode", "count_topo", "--samples", "samples.txt", "--mut", "P", "--chr", "chr.txt", "--seed", "5", "-o", out], cwd=d,
                       capture_output=True, text=True, env=env, timeout=3400)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("triples drawn on the device" if device else "triples drawn on the host") in r.stderr, r.stderr[-1500:]
    assert device == ("on the host" not in r.stderr), "no device: this measurement needs one\n" + r.stderr[-1500:]
    m = re.search("Timing: count_topo samples: inputs " + NUM + " s, triple stage " + NUM + r" s \(device kernels " + NUM + r" s\), files " + NUM
                  + r" s; (\d+) rows, (\d+) samples, (\d+) triples", r.stderr)
    assert m, r.stderr[-1500:]
    return {"wall_s": wall, "inputs_s": float(m.group(1)), "triple_stage_s": float(m.group(2)), "kernels_s": float(m.group(3)),
            "files_s": float(m.group(4)), "rows": int(m.group(5)), "samples": int(m.group(6)), "triples": int(m.group(7))}


def median_of(runs, key):
    return round(statistics.median(x[key] for x in runs), 4)


def measure(d, reps):
    def timed(what, out, device):  # (a line per run, so that a long measurement shows where it is)
        r = run(d, out, device)
        print(f"{what}: {r['wall_s']:.2f} s", file=sys.stderr, flush=True)
        return r

    timed("warm-up, device", "dev", True), timed("warm-up, host twin", "host", False)  # file cache, code objects
    dev, host = [], []
    for k in range(reps):  # (taking turns, and the form that goes first alternates too)
        for form in (("d", "h") if k % 2 == 0 else ("h", "d")):
            if form == "d":
                dev.append(timed("device", "dev", True))
            else:
                host.append(timed("host twin", "host", False))
    files = sorted(glob.glob(os.path.join(d, "dev_*.txt")) + [os.path.join(d, "dev.triples.txt")])
    same = len(files) == dev[0]["triples"] + 1 and all(
        open(f, "rb").read() == open(os.path.join(d, "host" + os.path.basename(f)[3:]), "rb").read() for f in files)
    out = {"files_equal_bytes": same, "rows": dev[0]["rows"], "samples": dev[0]["samples"], "triples": dev[0]["triples"]}
    for name, runs in (("device", dev), ("host_twin", host)):
        out[name] = {k + "_median": median_of(runs, k) for k in ("wall_s", "inputs_s", "triple_stage_s", "kernels_s", "files_s")}
        out[name]["wall_s_all"] = [round(x["wall_s"], 3) for x in runs]
        out[name]["triple_stage_s_all"] = [round(x["triple_stage_s"], 4) for x in runs]
    out["inputs_share_of_device_wall"] = round(out["device"]["inputs_s_median"] / out["device"]["wall_s_median"], 3)
    out["triple_stage_device_not_slower_than_host_twin"] = out["device"]["triple_stage_s_median"] <= out["host_twin"]["triple_stage_s_median"]
    out["device_not_slower_than_host_twin"] = out["device"]["wall_s_median"] <= out["host_twin"]["wall_s_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="6 samples over small synthetic files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.record is None:
        a.record = os.path.join(ROOT, "profiles", "topo", "count_topo_bench_small.json" if a.small else "count_topo_bench.json")
    own = a.workdir is None
    if own:
        a.workdir = tempfile.mkdtemp(prefix="count_topo_bench_")
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
                     else f"{len(files)} samples, 22 chromosomes x 1 M .mut rows (BASELINE configs[4])") + f"; 2 cond x {len(targets)} targets x {len(refs)} references, three different lines each", "reps": a.reps}
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
