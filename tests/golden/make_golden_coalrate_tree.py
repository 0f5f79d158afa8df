"""Regenerates tests/golden/crtree_*/ (TEST INFRASTRUCTURE): synthetic inputs (tests/condcoal_synth.py) and the
reference's `CoalRate --mode tree` output for them.

The recipe of make_golden_coalrate.py: the reference's CoalRate is compiled from REF (default /root/reference) into a
temporary directory outside the repository and run there; only the inputs, case.json and its .coal output are kept.
Every case is run twice and refused when the two outputs differ.

    python tests/golden/make_golden_coalrate_tree.py [--ref /root/reference] [--only NAME]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import condcoal_synth as cs  # noqa: E402
from make_golden_coalrate import build_reference  # noqa: E402


def quantised_tree_fn(rng, quantum=64.0):
    """tree_fn for write_chromosome: coalescences in label order at heights that are multiples of `quantum`, a step of 0
    now and then, so that internal nodes tie with each other and (ages being multiples too) with sample ages."""
    def fn(N, ages):
        ages = np.zeros(N) if ages is None else np.asarray(ages, float)
        heights = np.zeros(2 * N - 1)
        heights[:N] = ages
        parent = np.full(2 * N - 1, -1, dtype=np.int64)
        waiting = sorted(range(N), key=lambda i: (ages[i], i))
        active = []
        t = 0.0
        for label in range(N, 2 * N - 1):
            t += quantum * int(rng.integers(0, 3))
            while True:
                while waiting and ages[waiting[0]] <= t:
                    active.append(waiting.pop(0))
                if len(active) >= 2:
                    break
                t += quantum
            i, j = sorted(rng.choice(len(active), size=2, replace=False), reverse=True)
            a, b = active.pop(int(i)), active.pop(int(j))
            parent[a] = parent[b] = label
            heights[label] = t
            active.append(label)
        return parent, heights
    return fn


def make_case(name, out_dir, rng):
    os.makedirs(out_dir, exist_ok=True)
    args = ["--mode", "tree", "-i", "in", "-o", "out", "--bins", "3,6.5,0.5"]
    if name == "modern":
        cs.write_chromosome(os.path.join(out_dir, "in_chr1"), rng, 40, 30, span=3_000_000)
    elif name == "ancient":
        ages = np.zeros(24)
        ages[[2, 3]] = 20.0      # epoch 0 (below 10^3 / 28 = 35.7 generations)
        ages[[8, 9]] = 60.0      # epoch 1 (35.7 .. 112.9)
        ages[[14, 15]] = 200.0   # epoch 2 (112.9 .. 357.1)
        cs.write_chromosome(os.path.join(out_dir, "in_chr1"), rng, 24, 25, ages=ages, span=3_000_000, Ne=20000.0)
    elif name == "chr":
        with open(os.path.join(out_dir, "chr.txt"), "w") as f:
            f.write("1\n2\nX\n")
        for c in ("1", "2", "X"):
            cs.write_chromosome(os.path.join(out_dir, f"in_chr{c}"), rng, 16, 14, span=2_000_000)
        args += ["--chr", "chr.txt", "--num_bootstraps", "5"]
    elif name == "blocks":
        with open(os.path.join(out_dir, "chr.txt"), "w") as f:
            f.write("1\n2\n")
        ages = np.array([0.0, 0.0, 20.0, 0.0, 60.0, 0.0])
        cs.write_chromosome(os.path.join(out_dir, "in_chr1"), rng, 6, 5003, ages=ages)
        cs.write_chromosome(os.path.join(out_dir, "in_chr2"), rng, 6, 12, ages=ages, span=2_000_000)
        args += ["--chr", "chr.txt", "--num_bootstraps", "4"]
    elif name == "ties":
        ages = np.zeros(16)
        ages[[5, 11]] = 128.0
        ages[7] = 256.0
        cs.write_chromosome(os.path.join(out_dir, "in_chr1"), rng, 16, 20, ages=ages, span=2_000_000,
                            tree_fn=quantised_tree_fn(rng))
    elif name == "settings":
        cs.write_chromosome(os.path.join(out_dir, "in_chr1"), rng, 30, 20, span=2_000_000)
        args[args.index("--bins") + 1] = "2,7.95,0.05"
        args += ["--years_per_gen", "25", "--seed", "9"]
    else:
        raise SystemExit(f"unknown case {name}")
    with open(os.path.join(out_dir, "case.json"), "w") as f:
        json.dump({"args": args}, f)
        f.write("\n")
    return args


CASES = ["modern", "ancient", "chr", "blocks", "ties", "settings"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only")
    opt = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="coalrate_ref_") as tmp:
        exe = build_reference(opt.ref, tmp)
        for k, name in enumerate(CASES):
            if opt.only and name != opt.only:
                continue
            out_dir = os.path.join(HERE, f"crtree_{name}")
            if os.path.isdir(out_dir):
                shutil.rmtree(out_dir)
            args = make_case(name, out_dir, np.random.default_rng(5200 + k))
            outs = []
            for rep in range(2):
                run_dir = os.path.join(tmp, f"{name}_{rep}")
                shutil.copytree(out_dir, run_dir)
                subprocess.run([exe] + args, cwd=run_dir, check=True, capture_output=True)
                with open(os.path.join(run_dir, "out.coal")) as f:
                    outs.append(f.read())
            if outs[0] != outs[1]:
                raise SystemExit(f"case {name}: two runs of the reference differ (the fixture is refused)")
            with open(os.path.join(out_dir, "expected.coal"), "w") as f:
                f.write(outs[0])
            print(name, "ok:", len(outs[0].splitlines()), "lines")


if __name__ == "__main__":
    main()
