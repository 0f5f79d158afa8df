"""Regenerates tests/golden/coalrate_*/ (TEST INFRASTRUCTURE): synthetic inputs (tests/condcoal_synth.py) and the
reference's `CoalRate --mode local_ancestry` output for them.

The reference's CoalRate is compiled from REF (default /root/reference) into a temporary directory outside the repository
and run there; only the inputs and its .coal outputs are kept.  Every case is run twice and refused when the two outputs
differ: at the last tree of a chromosome the reference reads one element past its mutation list, and a case whose result
depended on that read would not be a fixture.

    python tests/golden/make_golden_coalrate.py [--ref /root/reference] [--only NAME]
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
import condcoal_synth as cs  # noqa: E402

SOURCES = ["coal/CoalRate.cpp", "coal/coal_EM.cpp", "coal/coal_tree.cpp", "coal/coal_EM_old.cpp", "src/data.cpp", "src/sample.cpp",
           "src/anc.cpp", "src/mutations.cpp", "src/gzstream/gzstream.cpp"]
INCLUDES = ["src", "src/gzstream", "src/tskit", "vcf", "coal", "test"]


def build_reference(ref, tmp):
    inc = os.path.join(ref, "include")
    exe = os.path.join(tmp, "CoalRate_ref")
    cmd = ["g++", "-O3", "-std=c++14"] + [f"-I{os.path.join(inc, d)}" for d in INCLUDES] + [os.path.join(inc, s) for s in SOURCES]
    cmd += ["-o", exe, "-lz", "-Wl,--unresolved-symbols=ignore-all"]
    subprocess.check_call(cmd)
    return exe


def mut_positions(prefix):
    import gzip
    with gzip.open(prefix + ".mut.gz", "rt") as f:
        rows = f.read().splitlines()[1:]
    return [(int(r.split(";")[1]), int(r.split(";")[4])) for r in rows]


def tree_spans(prefix):
    """(bp_start, bp_end) of every tree with SNPs, between SNP midpoints (coal.cpp:497-509)."""
    snps = mut_positions(prefix)
    spans = []
    i = 0
    while i < len(snps):
        j = i
        while j < len(snps) and snps[j][1] == snps[i][1]:
            j += 1
        start = snps[i][0] if i == 0 else (snps[i][0] + snps[i - 1][0]) // 2
        end = snps[-1][0] if j == len(snps) else (snps[j][0] + snps[j - 1][0]) // 2
        spans.append((start, end))
        i = j
    return spans


def write_local_ancestry(path, labels, rows):
    with open(path, "w") as f:
        f.write(" ".join(labels) + "\n")
        for chrom, bp, grp in rows:
            f.write(f"{chrom} {bp} " + " ".join(str(int(g)) for g in grp) + "\n")


def breakpoints(prefix, rng):
    """Segment starts that leave trees uncut, cut one once and cut one several times; none within the last three trees."""
    sp = tree_spans(prefix)
    assert len(sp) >= 12
    bps = []
    a, b = sp[2]
    bps.append((a + b) // 2)                       # cuts tree 2 once
    a, b = sp[5]
    third = max(1, (b - a) // 4)
    bps += [a + third, a + 2 * third, a + 3 * third]  # cuts tree 5 three times
    bps.append(sp[8][0])                           # a segment that starts where a tree starts
    bps = sorted(set(x for x in bps if 0 < x < sp[-3][0]))
    return bps


def make_case(name, out_dir, rng):
    os.makedirs(out_dir, exist_ok=True)
    args = ["--mode", "local_ancestry", "-i", "in", "-o", "out", "--poplabels", "pop.txt", "--bins", "3,6.5,0.5"]
    if name == "modern":
        cs.write_chromosome(os.path.join(out_dir, "in"), rng, 40, 30, span=3_000_000)
        cs.write_poplabels(os.path.join(out_dir, "pop.txt"), 40, 4, rng)
    elif name == "ancient":
        ages = np.zeros(24)
        ages[[2, 3]] = 20.0      # epoch 0 (below 10^3 / 28 = 35.7 generations)
        ages[[8, 9]] = 60.0      # epoch 1 (35.7 .. 112.9)
        ages[[14, 15]] = 200.0   # epoch 2 (112.9 .. 357.1)
        cs.write_chromosome(os.path.join(out_dir, "in"), rng, 24, 25, ages=ages, span=3_000_000, Ne=20000.0)
        cs.write_poplabels(os.path.join(out_dir, "pop.txt"), 24, 3, rng)
    elif name == "chr":
        with open(os.path.join(out_dir, "chr.txt"), "w") as f:
            f.write("1\n2\nX\n")
        for c in ("1", "2", "X"):
            cs.write_chromosome(os.path.join(out_dir, f"in_chr{c}"), rng, 16, 14, span=2_000_000)
        cs.write_poplabels(os.path.join(out_dir, "pop.txt"), 16, 3, rng)
        args += ["--chr", "chr.txt", "--num_bootstraps", "5"]
    elif name == "localanc":
        with open(os.path.join(out_dir, "chr.txt"), "w") as f:
            f.write("1\n2\n")
        labels = ["AFR", "EUR", "NAT"]
        rows = []
        for c in ("1", "2"):
            prefix = os.path.join(out_dir, f"in_chr{c}")
            cs.write_chromosome(prefix, rng, 20, 16, span=2_000_000, no_snp_frac=0.0)
            rows.append((c, 0, rng.integers(0, 3, 20)))
            for bp in breakpoints(prefix, rng):
                rows.append((c, bp, rng.integers(0, 3, 20)))
        write_local_ancestry(os.path.join(out_dir, "pop.txt"), labels, rows)
        args += ["--chr", "chr.txt", "--num_bootstraps", "3"]
    elif name == "large":
        cs.write_chromosome(os.path.join(out_dir, "in"), rng, 300, 8, span=1_000_000, caterpillar=None, shuffled=2)
        cs.write_poplabels(os.path.join(out_dir, "pop.txt"), 300, 16, rng)
    elif name == "settings":
        cs.write_chromosome(os.path.join(out_dir, "in"), rng, 30, 20, span=2_000_000)
        cs.write_poplabels(os.path.join(out_dir, "pop.txt"), 30, 3, rng)
        args[args.index("--bins") + 1] = "2,7.95,0.05"
        args += ["--years_per_gen", "25", "--seed", "9"]
    else:
        raise SystemExit(f"unknown case {name}")
    with open(os.path.join(out_dir, "case.json"), "w") as f:
        json.dump({"args": args}, f)
        f.write("\n")
    return args


CASES = ["modern", "ancient", "chr", "localanc", "large", "settings"]


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
            out_dir = os.path.join(HERE, f"coalrate_{name}")
            if os.path.isdir(out_dir):
                shutil.rmtree(out_dir)
            args = make_case(name, out_dir, np.random.default_rng(4100 + k))
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
