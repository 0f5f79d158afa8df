"""Writes the `Colate --mode CondCoalRates --pairs` fixtures under tests/golden/ccpairs_<case>/ (TEST INFRASTRUCTURE; runs
only where oracle/_ref/Colate_ref was built from the reference, like make_golden_condcoal.py): synthetic inputs from
tests/condcoal_synth.py, the list of pairs (pairs.txt, `FOCAL,COND expected_<k>.txt` per line) and the reference's table of
every pair, each from its own single run (`--groups FOCAL,COND`).  case.json holds the shared command-line arguments
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

# name: (seed, N, trees per chromosome, chromosomes, ancient, groups, span, extra arguments, absent conditional group)
CASES = {
    "modern5": (31, 30, 40, None, False, 5, 70_000_000, ["--bins", "3,5,0.5", "--lineage_bin", "4"], "PZ"),
    "ancient": (32, 30, 40, None, True, 3, 40_000_000, ["--lineage_bin", "4"], "PQ"),
    "chr_boot": (33, 24, 30, ["1", "2"], False, 3, 35_000_000,
                 ["--bins", "3,5,0.5", "--lineage_bin", "4", "--num_bootstraps", "3", "--seed", "7"], "PZ"),
}


def make_case(name):
    seed, N, T, chroms, ancient, ngroups, span, extra, absent = CASES[name]
    d = os.path.join(HERE, f"ccpairs_{name}")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    rng = np.random.default_rng(seed)
    ages = cs.ancient_ages(rng, N) if ancient else None
    cs.write_poplabels(os.path.join(d, "in.poplabels"), N, ngroups, rng)
    args = ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels"] + extra
    if chroms:
        with open(os.path.join(d, "chr.txt"), "w") as f:
            f.write("".join(c + "\n" for c in chroms))
        for c in chroms:
            cs.write_chromosome(os.path.join(d, f"in_chr{c}"), rng, N, T, ages, span=span, caterpillar=3, shuffled=5)
        args += ["--chr", "chr.txt"]
    else:
        cs.write_chromosome(os.path.join(d, "in"), rng, N, T, ages, span=span, caterpillar=3, shuffled=5)
    with open(os.path.join(d, "in.poplabels")) as f:
        groups = sorted({line.split()[1] for line in f.read().splitlines()[1:] if line.strip()})
    pairs = [f"{a},{b}" for a in groups for b in groups] + [f"{groups[0]},{absent}"]
    lines = []
    for k, g in enumerate(pairs):
        out = f"expected_{k}.txt"
        r = subprocess.run([REF] + args + ["--groups", g, "--output", out], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, (name, g, r.returncode, r.stderr[-2000:])
        lines.append(f"{g} {out}\n")
    with open(os.path.join(d, "pairs.txt"), "w") as f:
        f.write("".join(lines))
    with open(os.path.join(d, "case.json"), "w") as f:
        json.dump({"args": args, "N": N, "ancient": ancient, "pairs": len(pairs)}, f, indent=1)
    print(name, len(pairs), "pairs ok")


if __name__ == "__main__":
    assert os.path.exists(REF), f"{REF} missing: build it with `make -C oracle ref`"
    for n in (sys.argv[1:] or CASES):
        make_case(n)
