#!/usr/bin/env python3
"""Generates tests/golden/pairs_masks/ from the REFERENCE ITSELF: `Colate --pairs` lines with per-pair masks and .coal warm
starts (target_mask=, reference_mask=, coal=), against oracle/_ref/Colate_ref run once per pair with the matching
--target_mask / --reference_mask / --coal options (the reference has no list mode).

Four samples (T, T1, R, R1) over one set of .mut files, a FASTA mask per sample and chromosome (one lower-case, one shorter than
its chromosome), and the warm start of l3_coal_modern (prev.coal, more epochs than --bins 3,7,0.2: a second launch).  The
directory is not named l3_*: the single-pair tests iterate over those.

The fixture is data (inputs and expected outputs); no reference source is copied.  Needs oracle/_ref/Colate_ref
(make -C oracle ref).
    python tests/golden/make_golden_pairs_masks.py
"""
import gzip
import json
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (run_ref, _isnum; importing it generates nothing)
import synth_files  # noqa: E402

OUT = os.path.join(HERE, "pairs_masks")
SPAN = 3_000_000


def mask_text(n, seed, lower=False):
    """make_golden.make_l3's mask style: runs of P (callable) and N, some in lower case (the reader upper-cases)."""
    r = np.random.default_rng(seed)
    seq = []
    while sum(len(x) for x in seq) < n:
        seq.append(("p" if lower and r.uniform() < 0.3 else "P") * int(r.integers(20_000, 120_000)))
        seq.append(("N" if r.uniform() < 0.7 else "n") * int(r.integers(5_000, 40_000)))
    seq = "".join(seq)[:n]
    return ">mask\n" + "\n".join(seq[i:i + 100] for i in range(0, n, 100)) + "\n"


# (target, reference, output, target_age, reference_age or None, keys)
PAIRS = [
    ("T.colate.in", "R.colate.in", "p0", None, None, {"target_mask": "TM", "reference_mask": "RM"}),  # both masks
    ("T1.colate.in", "R.colate.in", "p1", None, None, {"target_mask": "TM1"}),  # the target mask only
    ("T.colate.in", "R1.colate.in", "p2", None, None, {}),  # no mask
    ("T.colate.in", "R1.colate.in", "p3", "0", "0", {"reference_mask": "RM1", "target_mask": "TM"}),  # TM shared with p0
    ("T1.colate.in", "R.colate.in", "p4", None, None, {"coal": "prev.coal"}),  # modern warm start
    ("T1.colate.in", "R1.colate.in", "p5", "7000", "0", {"coal": "prev.coal"}),  # ancient warm start (age inserted)
    ("R.colate.in", "T.colate.in", "p6", None, None, {"target_mask": "RM", "reference_mask": "TM", "coal": "prev.coal"}),
]
COMMON = ["--bins", "3,7,0.2", "--seed", "13", "--num_bootstraps", "3", "--chr", "chr.txt"]
OPTION = {"target_mask": "--target_mask", "reference_mask": "--reference_mask", "coal": "--coal"}


def main():
    assert os.path.exists(mg.REF_BIN), "oracle/_ref/Colate_ref missing: make -C oracle ref"
    shutil.rmtree(OUT, ignore_errors=True)
    synth_files.write_inputs(OUT, chroms=("1", "2"), snps_per_chr=900, seed=51, gz=True, span=SPAN, extra_targets=1, extra_refs=1)
    masks = {"TM_chr1.fa": mask_text(SPAN, 61), "TM_chr2.fa": mask_text(SPAN, 62, lower=True),
             "TM1_chr1.fa": mask_text(SPAN, 63), "TM1_chr2.fa": mask_text(SPAN, 64),
             "RM_chr1.fa": mask_text(SPAN, 65, lower=True), "RM_chr2.fa": mask_text(2_000_000, 66),  # shorter than chromosome 2
             "RM1_chr1.fa": mask_text(SPAN, 67), "RM1_chr2.fa": mask_text(SPAN, 68, lower=True)}
    for fn, text in masks.items():  # the readers fall back to <name>.gz
        with gzip.GzipFile(os.path.join(OUT, fn + ".gz"), "wb", mtime=0) as g:
            g.write(text.encode())
    shutil.copy(os.path.join(HERE, "l3_coal_modern", "prev.coal"), os.path.join(OUT, "prev.coal"))
    meta = {"generator": "tests/golden/make_golden_pairs_masks.py (oracle/_ref/Colate_ref, one run per pair)",
            "common_args": COMMON, "pairs": []}
    for tgt, ref, out, ta, ra, keys in PAIRS:
        args = ["--mode", "mut", "--mut", "P", "--target_tmp", tgt, "--reference_tmp", ref]
        if ta is not None:
            args += ["--target_age", ta, "--reference_age", ra]
        for k, v in keys.items():
            args += [OPTION[k], v]
        args += COMMON + ["-o", "expected_" + out]
        err, iters = mg.run_ref(args, OUT)
        nblocks = int(re.search(r"Number of blocks: (\d+)", err).group(1))
        p = {"target": tgt, "reference": ref, "output": out, "target_age": ta, "reference_age": ra, "keys": keys, "args": args,
             "iterations": iters, "num_blocks": nblocks}
        if "coal" in keys:  # the starting rates the reference printed (coal.cpp:3642)
            line = [l for l in err.split("\n") if l.strip() and all(mg._isnum(t) for t in l.split())]
            p["init_rates_printed"] = line[-1].split()
        meta["pairs"].append(p)
        print(f"pairs_masks {out}: blocks={nblocks} iterations={iters}")
    json.dump(meta, open(os.path.join(OUT, "case.json"), "w"), indent=1)
    for fn in sorted(os.listdir(OUT)):  # keep the fixture small
        if fn.endswith(".colate.in"):
            with open(os.path.join(OUT, fn), "rb") as f, gzip.GzipFile(os.path.join(OUT, fn + ".gz"), "wb", mtime=0) as g:
                g.write(f.read())
            os.remove(os.path.join(OUT, fn))


if __name__ == "__main__":
    main()
