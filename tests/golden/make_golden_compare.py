#!/usr/bin/env python3
"""Generates tests/golden/compare_tmp/ from the REFERENCE ITSELF: `Colate --mode compare_tmp` (oracle/_ref/Colate_ref), one
run per pair.

Four samples (T, T1, R, R1) over three chromosomes of about 900 rows each, 95 Mb long (ten 10 Mb windows), gzipped; a quarter
of chromosome 2's rows written twice (rows at equal positions).  The pairs are those of the sample list SAMPLES -- both orders
of (T, R) among them -- so that `--samples` can be compared file by file.  nochr/: one .mut file without --chr, the empty
chromosome name (the cursor path).

The fixture is data (inputs and expected outputs); no reference source is copied.  Needs oracle/_ref/Colate_ref
(make -C oracle ref).
    python tests/golden/make_golden_compare.py
"""
import gzip
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (run_ref; importing it generates nothing)
import synth_files  # noqa: E402

OUT = os.path.join(HERE, "compare_tmp")
# the list of the tests: NAME FILE [role=]; its pairs are every (target line, reference line) of different lines
SAMPLES = ["a T.colate.in", "b T1.colate.in role=target", "c R.colate.in", "d R1.colate.in role=reference"]


def pairs_of(samples):
    rows = [(s.split()[0], s.split()[1], s.split()[2] if len(s.split()) > 2 else "") for s in samples]
    return [(t, r) for t in rows for r in rows if t is not r and t[2] != "role=reference" and r[2] != "role=target"]


def gz_tmp_files(d):
    for fn in sorted(os.listdir(d)):  # keep the fixture small
        if fn.endswith(".colate.in"):
            with open(os.path.join(d, fn), "rb") as f, gzip.GzipFile(os.path.join(d, fn + ".gz"), "wb", mtime=0) as g:
                g.write(f.read())
            os.remove(os.path.join(d, fn))


def main():
    assert os.path.exists(mg.REF_BIN), "oracle/_ref/Colate_ref missing: make -C oracle ref"
    shutil.rmtree(OUT, ignore_errors=True)
    synth_files.write_inputs(OUT, chroms=("1", "2", "3"), snps_per_chr=900, seed=71, gz=True, extra_targets=1, extra_refs=1)
    synth_files.duplicate_rows(os.path.join(OUT, "P_chr2.mut.gz"), np.random.default_rng(72), 0.25)
    meta = {"generator": "tests/golden/make_golden_compare.py (oracle/_ref/Colate_ref, one run per pair)", "samples": SAMPLES, "pairs": []}
    for t, r in pairs_of(SAMPLES):
        out = f"expected_{t[0]}_{r[0]}.txt"
        args = ["--mode", "compare_tmp", "--mut", "P", "--target_tmp", t[1], "--reference_tmp", r[1], "--chr", "chr.txt", "--seed", "5", "-o", out]
        mg.run_ref(args, OUT)
        lines = open(os.path.join(OUT, out)).read().split("\n")
        meta["pairs"].append({"target": t[1], "reference": r[1], "names": [t[0], r[0]], "output": out, "args": args})
        print(f"compare_tmp {out}: {len(lines) - 1} lines")
    json.dump(meta, open(os.path.join(OUT, "case.json"), "w"), indent=1)
    gz_tmp_files(OUT)
    # ---- no --chr: one .mut file, the empty chromosome name
    sub = os.path.join(OUT, "nochr")
    synth_files.write_inputs(sub, chroms=("1",), snps_per_chr=700, seed=73, gz=True, span=45_000_000, with_chr_file=False)
    args = ["--mode", "compare_tmp", "--mut", "P.mut", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--seed", "5", "-o", "expected.txt"]
    mg.run_ref(args, sub)
    json.dump({"args": args}, open(os.path.join(sub, "case.json"), "w"), indent=1)
    print(f"compare_tmp nochr: {len(open(os.path.join(sub, 'expected.txt')).read().splitlines())} lines")
    gz_tmp_files(sub)


if __name__ == "__main__":
    main()
