"""Writes the `Colate --mode CondCoalRates` fixtures under tests/golden/condcoal_<case>/ (TEST INFRASTRUCTURE; runs
only where oracle/_ref/Colate_ref was built from the reference, like make_golden.py): synthetic inputs from
tests/condcoal_synth.py and the reference's output table, expected.txt.  case.json holds the command-line arguments
(paths relative to the case directory)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import condcoal_synth as cs  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "Colate_ref")

# name: (seed, N, trees per chromosome, chromosomes, ancient, groups, span, mask, extra arguments)
CASES = {
    "modern": (11, 40, 60, None, False, 4, 40_000_000, False, ["--groups", "PB,PC", "--lineage_bin", "4"]),
    "ancient": (12, 40, 60, None, True, 3, 40_000_000, False, ["--groups", "PA,PB", "--lineage_bin", "4"]),
    "empty_cond": (13, 30, 40, None, False, 3, 40_000_000, False, ["--groups", "PA,PZ", "--lineage_bin", "4"]),
    "empty_cond_ancient": (14, 30, 40, None, True, 3, 40_000_000, False, ["--groups", "PC,PZ", "--lineage_bin", "4"]),
    "same_group": (15, 30, 40, None, False, 5, 40_000_000, False, ["--groups", "PB,PB", "--lineage_bin", "4"]),
    "default_lineage": (16, 30, 40, None, False, 3, 40_000_000, False, ["--groups", "PA,PC"]),
    "bins": (17, 30, 40, None, False, 4, 40_000_000, False, ["--groups", "PA,PD", "--bins", "3,5,0.5", "--lineage_bin", "4"]),
    "chr": (18, 24, 30, ["1", "2"], False, 3, 35_000_000, False, ["--groups", "PA,PB", "--lineage_bin", "4"]),
    "mask": (19, 24, 40, None, False, 3, 3_000_000, True, ["--groups", "PB,PA", "--lineage_bin", "4"]),
    "boot": (20, 24, 60, None, False, 3, 100_000_000, False,
             ["--groups", "PA,PB", "--lineage_bin", "4", "--num_bootstraps", "5", "--seed", "3"]),
    "large": (21, 300, 3, None, False, 16, 40_000_000, False, ["--groups", "PC,PA", "--lineage_bin", "4"]),
}


def make_case(name):
    seed, N, T, chroms, ancient, ngroups, span, mask, extra = CASES[name]
    d = os.path.join(HERE, f"condcoal_{name}")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    rng = np.random.default_rng(seed)
    ages = cs.ancient_ages(rng, N) if ancient else None
    cs.write_poplabels(os.path.join(d, "in.poplabels"), N, ngroups, rng)
    args = ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels", "--output", "out.txt"] + extra
    if chroms:
        with open(os.path.join(d, "chr.txt"), "w") as f:
            f.write("".join(c + "\n" for c in chroms))
        for c in chroms:
            cs.write_chromosome(os.path.join(d, f"in_chr{c}"), rng, N, T, ages, span=span, caterpillar=3, shuffled=5)
        args += ["--chr", "chr.txt"]
    else:
        cs.write_chromosome(os.path.join(d, "in"), rng, N, T, ages, span=span, caterpillar=3, shuffled=5)
    if mask:
        cs.write_mask(os.path.join(d, "mask.fa"), span + 1000, rng)
        args += ["--mask", "mask.fa"]
    r = subprocess.run([REF] + args, cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    os.replace(os.path.join(d, "out.txt"), os.path.join(d, "expected.txt"))
    with open(os.path.join(d, "case.json"), "w") as f:
        json.dump({"args": args, "N": N, "ancient": ancient}, f, indent=1)
    print(name, "ok")


if __name__ == "__main__":
    assert os.path.exists(REF), f"{REF} missing: build it with `make -C oracle ref`"
    for n in (sys.argv[1:] or CASES):
        make_case(n)
