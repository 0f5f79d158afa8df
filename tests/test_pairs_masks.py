"""`Colate --pairs` lines with per-pair masks and .coal warm starts (`target_mask=`, `reference_mask=`, `coal=`), on the CPU
(--counts_only): the list grammar, the masks decoded once per file, masked pairs through the walk indices, and the tables against
the single-pair CLI and -- through the oracle's EM -- against the reference run once per pair (fixture pairs_masks)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import golden_lib as gl
import oracle_lib as ol
import pairs_masks_lib as pm
import synth_files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")
OPTION = {"target_mask": "--target_mask", "reference_mask": "--reference_mask", "coal": "--coal"}


def _run(args, cwd, **env):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)


def _common(meta):
    return ["--mode", "mut", "--mut", "P"] + meta["common_args"]


def test_masked_list_counts_equal_single_pair_runs(tmp_path):
    """Every line of the list -- both masks, one mask, none, masks shared between pairs, coal= with and without masks -- gives the
    count tables of the single-pair CLI with the matching --target_mask / --reference_mask / --coal and the same seed, through the
    sequential feeder (COLATE_THREADS=1, the reference's order); the masked pairs walk through the indices."""
    meta = pm.stage(tmp_path)
    common = _common(meta)
    r = _run(common + ["--pairs", "pairs.txt", "--counts_only"], tmp_path, COLATE_TIMING="1")
    assert r.returncode == 0, r.stderr[-800:]
    n_masked = sum(1 for p in meta["pairs"] if "target_mask" in p["keys"] or "reference_mask" in p["keys"])
    assert f"{len(meta['pairs'])} of {len(meta['pairs'])} pairs walked through indices ({n_masked} masked)" in r.stderr, r.stderr[-1500:]
    for p in meta["pairs"]:
        assert f"{p['target']} x {p['reference']}: Number of blocks: {p['num_blocks']}" in r.stderr
        single = ["--target_tmp", p["target"], "--reference_tmp", p["reference"]]
        if p["target_age"] is not None:
            single += ["--target_age", p["target_age"], "--reference_age", p["reference_age"]]
        for k, v in p["keys"].items():
            single += [OPTION[k], v]
        out = p["output"] + "_single"
        s = _run(common + single + ["-o", out, "--counts_out", out + ".counts", "--counts_only"], tmp_path, COLATE_THREADS="1")
        assert s.returncode == 0, s.stderr[-800:]
        assert (tmp_path / (p["output"] + ".counts")).read_text() == (tmp_path / (out + ".counts")).read_text(), p["output"]


def test_masked_list_reproduces_reference_through_the_oracle(tmp_path):
    """Against the REFERENCE (pairs_masks: Colate_ref once per pair with the same masks and warm starts): each pair's count tables,
    through the oracle's EM from the pair's own epochs and starting rates, print exactly the reference's .coal with its iteration
    counts; the starting rates each warm-started pair prints are those the reference printed."""
    meta = pm.stage(tmp_path)
    common = _common(meta)
    B = int(common[common.index("--num_bootstraps") + 1])
    r = _run(common + ["--pairs", "pairs.txt", "--counts_only"], tmp_path)
    assert r.returncode == 0, r.stderr[-800:]
    bins = common[common.index("--bins") + 1]
    for k, p in enumerate(meta["pairs"]):
        if "coal" in p["keys"]:
            printed = [l for l in r.stderr.split("\n") if l.startswith(f"Pair {k + 1}: ")]
            assert len(printed) == 1 and printed[0].split()[2:] == p["init_rates_printed"], (p["output"], printed)
        grid, csh, cns = gl.read_counts(tmp_path / (p["output"] + ".counts"), B)
        ep, ep_null, kw = pm.epochs_of(p, bins, tmp_path)
        rates, iters, ll, fl = ol.em_batch(grid, csh, cns, ep, **kw)
        assert iters.tolist() == p["iterations"], p["output"]
        age = pm.age_of(p)
        assert gl.coal_text(ep, rates, age > 0, ep_null) == (tmp_path / f"expected_{p['output']}.coal").read_text(), p["output"]


def test_mask_key_is_applied_not_dropped(tmp_path):
    """`T R out 0 0 target_mask=TM` removes rows: its tables differ from the same line without the key."""
    pm.stage(tmp_path)
    (tmp_path / "two.txt").write_text("T.colate.in R.colate.in with 0 0 target_mask=TM\nT.colate.in R.colate.in without 0 0\n")
    r = _run(["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "3", "--num_bootstraps", "2",
              "--pairs", "two.txt", "--counts_only"], tmp_path)
    assert r.returncode == 0, r.stderr[-800:]
    _, sh1, ns1 = gl.read_counts(tmp_path / "with.counts", 2)
    _, sh2, ns2 = gl.read_counts(tmp_path / "without.counts", 2)
    assert (sh1 + ns1).sum() < 0.9 * (sh2 + ns2).sum()


def test_masked_counts_do_not_depend_on_the_walk(tmp_path):
    """The same tables with the cursor walk (COLATE_INDEXED_WALK=0) and with one worker (COLATE_THREADS=1); only the default run
    walks through indices."""
    meta = pm.stage(tmp_path)
    common = _common(meta) + ["--pairs", "pairs.txt", "--counts_only"]
    outs = [p["output"] + ".counts" for p in meta["pairs"]]
    runs = {}
    for name, env in (("indexed", {}), ("cursors", {"COLATE_INDEXED_WALK": "0"}), ("one_thread", {"COLATE_THREADS": "1"})):
        r = _run(common, tmp_path, COLATE_TIMING="1", **env)
        assert r.returncode == 0, r.stderr[-800:]
        m = re.search(r"(\d+) of (\d+) pairs walked through indices \((\d+) masked\)", r.stderr)
        assert m, r.stderr[-800:]
        n = len(meta["pairs"])
        assert (int(m.group(1)), int(m.group(2))) == ((0 if name == "cursors" else n), n), (name, m.group(0))
        runs[name] = [(tmp_path / o).read_text() for o in outs]
    assert runs["indexed"] == runs["cursors"] == runs["one_thread"]


def test_each_mask_file_is_decoded_once(tmp_path):
    """Six pairs over two masked samples (T with TM, R with RM, two chromosomes): four FASTA reads, whatever the number of pairs."""
    pm.stage(tmp_path)
    lines = [f"T.colate.in R.colate.in a{i} target_mask=TM reference_mask=RM\n" for i in range(3)]
    lines += [f"T.colate.in R1.colate.in b{i} target_mask=TM\n" for i in range(2)]
    lines += ["R.colate.in T1.colate.in c target_mask=RM\n"]
    (tmp_path / "six.txt").write_text("".join(lines))
    r = _run(["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "3", "--pairs", "six.txt", "--counts_only"],
             tmp_path, COLATE_TIMING="1")
    assert r.returncode == 0, r.stderr[-800:]
    assert "(2 masks decoded once: 4 FASTA reads)" in r.stderr, r.stderr[-800:]
    assert "6 of 6 pairs walked through indices (6 masked)" in r.stderr, r.stderr[-800:]
    assert (tmp_path / "a0.counts").read_text() == (tmp_path / "a2.counts").read_text()


@pytest.mark.parametrize("line, what", [
    ("T.colate.in R.colate.in x target_mask=TM colour=red", "unknown key 'colour'"),
    ("T.colate.in R.colate.in x target_mask=TM target_mask=TM1", "the key 'target_mask' is given twice"),
    ("T.colate.in R.colate.in x reference_mask=", "the key 'reference_mask' has no value"),
    ("T.colate.in R.colate.in x 0 0 0", "more than two ages"),
    ("T.colate.in R.colate.in x 0 TM_prefix", "the age 'TM_prefix' is not a number"),
    ("T.colate.in R.colate.in x 5abc", "the age '5abc' is not a number"),
])
def test_pair_list_errors_name_the_line(tmp_path, line, what):
    pm.stage(tmp_path)
    (tmp_path / "bad.txt").write_text("T.colate.in R.colate.in ok\n\n" + line + "\n")
    r = _run(["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "3", "--pairs", "bad.txt", "--counts_only"],
             tmp_path)
    assert r.returncode == 1 and f"bad.txt, line 3: {what}" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "ok.counts").exists()


def test_bins_needed_only_by_lines_without_coal(tmp_path):
    pm.stage(tmp_path)
    base = ["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--seed", "3", "--counts_only"]
    (tmp_path / "all.txt").write_text("T.colate.in R.colate.in a coal=prev.coal\nT1.colate.in R.colate.in b 7000 coal=prev.coal\n")
    r = _run(base + ["--pairs", "all.txt"], tmp_path)
    assert r.returncode == 0 and (tmp_path / "b.counts").exists(), r.stderr[-500:]
    (tmp_path / "some.txt").write_text("T.colate.in R.colate.in a coal=prev.coal\nT1.colate.in R.colate.in b\n")
    r = _run(base + ["--pairs", "some.txt"], tmp_path)
    assert r.returncode == 1 and "--bins" in r.stderr and "pair 2" in r.stderr, r.stderr[-500:]


def test_missing_mask_file_fails_like_the_single_pair_cli(tmp_path):
    """A missing mask file ends the run with exit 1 and the reference's message, naming the first missing file in the order the
    single-pair CLI opens them (chromosome by chromosome, target before reference) -- the same line every time, however the
    decoding is scheduled.  Here the second pair's target mask is missing on both chromosomes and the reference mask of
    chromosome 2 too: chromosome 1's NOPE file comes first."""
    pm.stage(tmp_path)
    os.remove(tmp_path / "RM_chr2.fa.gz")
    (tmp_path / "m.txt").write_text("T.colate.in R.colate.in a target_mask=TM reference_mask=RM\n"
                                    "T.colate.in R.colate.in b target_mask=NOPE reference_mask=RM\n")
    common = ["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "3", "--counts_only"]
    s = _run(common + ["--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--target_mask", "NOPE", "--reference_mask",
                       "RM", "-o", "single"], tmp_path, COLATE_THREADS="1")
    want = [l for l in s.stderr.split("\n") if l.startswith("Error")]
    assert s.returncode == 1 and want == ["Error while opening file NOPE_chr1.fa."], s.stderr[-500:]
    for threads in ("16", "16", "16", "2", "1"):
        r = _run(common + ["--pairs", "m.txt"], tmp_path, COLATE_THREADS=threads)
        got = [l for l in r.stderr.split("\n") if l.startswith("Error")]
        assert r.returncode == 1 and got == want, (threads, r.stderr[-500:])


# ---------------------------------------------------------------- randomised differential: indexed against cursor walk, masked pairs
def _sort_records(path, rng, dup_frac):
    """Rewrites a .colate.in with each chromosome's records in non-descending position order (the walk indices need that) and a
    fraction of them written twice with other counts (equal record positions)."""
    b = open(path, "rb").read()
    i, recs = 0, []
    while i + 4 <= len(b):
        (l,) = struct.unpack_from("<i", b, i)
        (bp,) = struct.unpack_from("<i", b, i + 4 + l)
        recs.append((b[i + 4:i + 4 + l], bp, b[i:i + 4 + l + 14]))
        i += 4 + l + 14
    order = {}
    for name, _, _ in recs:
        order.setdefault(name, len(order))
    recs.sort(key=lambda r: (order[r[0]], r[1]))  # (stable: equal positions keep their order)
    out = bytearray()
    for _, _, rec in recs:
        out += rec
        if rng.uniform() < dup_frac:
            out += rec[:-8] + struct.pack("<ii", int(rng.integers(0, 3)), int(rng.integers(0, 3)))
    open(path, "wb").write(bytes(out))


def _write_mask(path, n, rng, holes=(), lower=False):
    """Runs of P and N over n bases; `holes`: (begin, end) ranges set to N (a whole 30-Mb genome block)."""
    seq = np.empty(n, dtype="S1")
    k = 0
    while k < n:
        run = int(rng.integers(5_000, 400_000))
        seq[k:k + run] = b"P" if rng.uniform() < 0.7 else b"N"
        k += run
    for a, e in holes:
        seq[a:e] = b"N"
    text = seq.tobytes().decode()
    if lower:
        text = text.lower()
    with open(path, "w") as f:
        f.write(">mask\n")
        for i in range(0, n, 10_000):
            f.write(text[i:i + 10_000] + "\n")


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_masked_indexed_walk_equals_the_cursor_walk(tmp_path, seed):
    """Random masks (one of them removes the whole second genome block of chromosome 1, one is shorter than its chromosome, one in
    lower case), rows and records at equal positions, three targets x two references in several stream windows: the masked pairs'
    walk through the indices (TgtIdx of both samples and the pair's own last searches) finds exactly what the cursors find."""
    d = str(tmp_path)
    rng = np.random.default_rng(seed)
    span = 70_000_000
    synth_files.write_inputs(d, chroms=("1", "2"), snps_per_chr=5000, seed=seed, span=span, gz=True, extra_targets=2, extra_refs=1)
    for c in ("1", "2"):
        synth_files.duplicate_rows(os.path.join(d, f"P_chr{c}.mut.gz"), rng, 0.05)
    for f in ("T", "T1", "T2", "R", "R1"):
        _sort_records(os.path.join(d, f + ".colate.in"), rng, 0.03 if seed != 21 else 0.0)
    _write_mask(os.path.join(d, "MT_chr1.fa"), span, rng, holes=[(30_000_000, 60_000_000)])
    _write_mask(os.path.join(d, "MT_chr2.fa"), span, rng, lower=True)
    _write_mask(os.path.join(d, "MT1_chr1.fa"), span, rng)
    _write_mask(os.path.join(d, "MT1_chr2.fa"), 40_000_000, rng)  # (shorter than the chromosome: rows beyond it pass)
    _write_mask(os.path.join(d, "MR_chr1.fa"), span, rng)
    _write_mask(os.path.join(d, "MR_chr2.fa"), span, rng)
    masks = {"T": "target_mask=MT", "T1": "target_mask=MT1", "T2": ""}
    lines = []
    for t in ("T", "T1", "T2"):
        for r, rm in (("R", "reference_mask=MR"), ("R1", "")):
            lines.append(f"{t}.colate.in {r}.colate.in o_{t}_{r} {masks[t]} {rm}\n")
    (tmp_path / "pairs.txt").write_text("".join(lines))
    args = ["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "4", "--num_bootstraps", "2",
            "--pairs", "pairs.txt", "--counts_only"]
    outs = [ln.split()[2] + ".counts" for ln in lines]
    r = _run(args, d, COLATE_TIMING="1", COLATE_UNIFORM_WINDOW_MB="4", COLATE_INDEXED_WALK="0")
    assert r.returncode == 0 and "0 of 6 pairs walked through indices (5 masked)" in r.stderr, r.stderr[-800:]
    want = [(tmp_path / o).read_bytes() for o in outs]
    for o in outs:
        os.remove(tmp_path / o)
    r = _run(args, d, COLATE_TIMING="1", COLATE_UNIFORM_WINDOW_MB="4")
    assert r.returncode == 0 and "6 of 6 pairs walked through indices (5 masked)" in r.stderr, r.stderr[-800:]
    got = [(tmp_path / o).read_bytes() for o in outs]
    diff = [o for o, a, b in zip(outs, want, got) if a != b]
    assert diff == []
    assert len(set(want)) == len(outs)
