#!/usr/bin/env python3
"""Generates tests/golden/count_topo/ from the REFERENCE ITSELF: `Colate --mode count_topo` (oracle/_ref/Colate_ref), one run
per triple, all with --seed 5.

Five samples (T, T1, T2, R, R1) over three chromosomes of about 900 rows each, gzipped; a quarter of chromosome 2's rows
written twice (rows at equal positions).  The triples are those of the sample list SAMPLES -- both orders of the (b, c) pair
among them -- so that `--samples` can be compared file by file.  nochr/: one .mut file without --chr, the empty chromosome
name (the cursor path).

The generator ASSERTS that the fixture can tell a wrong implementation from a right one: every expected file has lines of both
signs; a printed row's position is absent from the cond file (the conditioning record is not the row's); a target or reference
has 1 < N and 0 < DAF < N at a printed row (the uniforms decide it); a searched row has age_begin == age_end.

The fixture is data (inputs and expected outputs); no reference source is copied.  Needs oracle/_ref/Colate_ref
(make -C oracle ref).
    python tests/golden/make_golden_topo.py
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
from make_golden_compare import gz_tmp_files  # noqa: E402

OUT = os.path.join(HERE, "count_topo")
SEED = "5"
# the list of the tests: NAME FILE [role=a,b]; its triples are every (cond line, target line, reference line) of three lines
SAMPLES = ["a T.colate.in role=cond,target", "b T1.colate.in role=target,reference", "c R.colate.in", "d R1.colate.in role=reference",
           "e T2.colate.in role=cond"]


def triples_of(samples):
    rows = []
    for s in samples:
        tok = s.split()
        roles = tok[2][len("role="):].split(",") if len(tok) > 2 else ["cond", "target", "reference"]
        rows.append((tok[0], tok[1], roles))
    return [(c, t, r) for c in rows for t in rows for r in rows
            if "cond" in c[2] and "target" in t[2] and "reference" in r[2] and c is not t and c is not r and t is not r]


def searched_rows(d, chrom):
    """(pos, anc/der, age_begin, age_end) of the rows the mode searches, as floats of the file's text"""
    out = []
    with gzip.open(os.path.join(d, f"P_chr{chrom}.mut.gz"), "rt") as f:
        next(f)
        for line in f:
            x = line.split(";")
            begin, end = np.float32(x[8]), np.float32(x[9])
            if x[7] == "0" and len(x[5].split()) == 1 and begin <= end and len(x[10]) == 3 and x[10][1] == "/":
                out.append((int(x[1]), x[10], begin, end))
    return out


def main():
    assert os.path.exists(mg.REF_BIN), "oracle/_ref/Colate_ref missing: make -C oracle ref"
    shutil.rmtree(OUT, ignore_errors=True)
    chroms = ("1", "2", "3")
    synth_files.write_inputs(OUT, chroms=chroms, snps_per_chr=900, seed=81, gz=True, extra_targets=2, extra_refs=1)
    synth_files.duplicate_rows(os.path.join(OUT, "P_chr2.mut.gz"), np.random.default_rng(82), 0.25)
    assert any(b == e for ch in chroms for _, _, b, e in searched_rows(OUT, ch)), "no searched row with age_begin == age_end"
    recs = {fn: {(r[0], r[1]): r for r in synth_files.read_records(os.path.join(OUT, fn))} for fn in os.listdir(OUT) if fn.endswith(".colate.in")}
    meta = {"generator": "tests/golden/make_golden_topo.py (oracle/_ref/Colate_ref, one run per triple)", "samples": SAMPLES, "seed": int(SEED),
            "triples": []}
    unmatched = decided = 0
    for c, t, r in triples_of(SAMPLES):
        out = f"expected_{c[0]}_{t[0]}_{r[0]}.txt"
        args = ["--mode", "count_topo", "--mut", "P", "-i", c[1], "--target_tmp", t[1], "--reference_tmp", r[1], "--chr", "chr.txt", "--seed", SEED,
                "-o", out]
        mg.run_ref(args, OUT)
        lines = [x.split() for x in open(os.path.join(OUT, out)).read().splitlines()]
        signs = [x[4] for x in lines]
        assert "1" in signs and "-1" in signs, (out, "lines of one sign only")
        for x in lines:
            key = (x[0], int(x[1]))
            unmatched += key not in recs[c[1]]
            for fn in (t[1], r[1]):
                aaf, daf = recs[fn][key][4], recs[fn][key][5]
                decided += aaf + daf > 1 and 0 < daf < aaf + daf
        meta["triples"].append({"cond": c[1], "target": t[1], "reference": r[1], "names": [c[0], t[0], r[0]], "output": out, "args": args,
                                "plus": signs.count("1"), "minus": signs.count("-1")})
        print(f"count_topo {out}: {len(lines)} lines")
    assert unmatched > 0, "every printed row's position is in the cond file"
    assert decided > 0, "no printed row at which the uniforms decide"
    print(f"printed rows absent from the cond file: {unmatched}; target / reference counts the uniforms decide: {decided}")
    json.dump(meta, open(os.path.join(OUT, "case.json"), "w"), indent=1)
    gz_tmp_files(OUT)
    # ---- no --chr: one .mut file, the empty chromosome name
    sub = os.path.join(OUT, "nochr")
    synth_files.write_inputs(sub, chroms=("1",), snps_per_chr=700, seed=83, gz=True, span=45_000_000, with_chr_file=False, extra_targets=1)
    args = ["--mode", "count_topo", "--mut", "P.mut", "-i", "T1.colate.in", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--seed",
            SEED, "-o", "expected.txt"]
    mg.run_ref(args, sub)
    signs = [x.split()[4] for x in open(os.path.join(sub, "expected.txt")).read().splitlines()]
    assert "1" in signs and "-1" in signs, "nochr: lines of one sign only"
    json.dump({"args": args}, open(os.path.join(sub, "case.json"), "w"), indent=1)
    print(f"count_topo nochr: {len(signs)} lines")
    gz_tmp_files(sub)


if __name__ == "__main__":
    main()
