"""The age sampling of the table fill on the GPU (colate_amd/csrc/fill_device.h, fill_kernel.hip; reference: coal.cpp:2260-2295)
against the same sampling on the host (csrc/mut_pairs.cpp, Engine::sample, itself pinned by the reference's fixtures in
tests/test_host_driver.py): the count tables must be the same bytes.  Through the C-ABI library's CLI entry point, as a user runs it."""
import os
import re
import subprocess

import pytest

import golden_lib as gl
import synth_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")


def _run(args, cwd, **env):
    e = dict(os.environ, COLATE_TIMING="1")
    e.update(env)
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, env=e, timeout=900)


def _redone(err):
    m = re.search(r"(\d+) pair\(s\) redone sequentially", err)
    assert m, err[-1500:]
    return int(m.group(1))


def _both_ways(args, cwd, outputs, redone=0, host_redone=None, **env):
    """Runs `args` with the sampling on the host, then on the device; returns (host files, device files, device stderr).  The
    device run must have handed exactly `redone` pairs back to the host (the host run `host_redone`, where given)."""
    r = _run(args, cwd, COLATE_DEVICE_FILL="0", **env)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    assert "age sampling on the host (COLATE_DEVICE_FILL=0)" in r.stderr.decode()
    if host_redone is not None:
        assert _redone(r.stderr.decode()) == host_redone, r.stderr.decode()[-1500:]
    host = {}
    for o in outputs:
        host[o] = open(os.path.join(cwd, o), "rb").read()
        os.remove(os.path.join(cwd, o))
    r = _run(args, cwd, **env)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    err = r.stderr.decode()
    m = re.search(r"age sampling on the GPU: (\d+) \(pair, block\) jobs, (\d+) SNPs in (\d+) launches", err)
    assert m, err[-1500:]  # (the device path must be the one that ran: no silent fall-back)
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0
    assert _redone(err) == redone, err[-1500:]
    dev = {o: open(os.path.join(cwd, o), "rb").read() for o in outputs}
    return host, dev, err


def test_pairs_fixture_tables_are_the_hosts(tmp_path):
    """The reference-made pairs fixture (modern pairs, a 500- and a 7000-year-old target; rows with age_begin = 0: the F path),
    one stream window and twelve (blocks that straddle hand-overs to the device)."""
    meta = gl.l3_pairs_stage(str(tmp_path))
    common = ["--mode", "mut", "--mut", "P"] + meta["common_args"]
    outs = [p["output"] + ".counts" for p in meta["pairs"]]
    for window in ("64", "4"):
        host, dev, err = _both_ways(common + ["--pairs", "pairs.txt", "--counts_only"], str(tmp_path), outs, COLATE_UNIFORM_WINDOW_MB=window)
        for o in outs:
            assert host[o] == dev[o], (o, window)


@pytest.mark.parametrize("name", ["l3_modern", "l3_ancient", "l3_nochr"])
def test_single_pair_cli_tables_are_the_hosts(name, tmp_path):
    """`Colate --mode mut` on one pair goes through the same engine (and so through the device)."""
    case = gl.l3_stage(name, str(tmp_path))
    args = [a for a in case["args"]]
    args[args.index("-o") + 1] = "mine"
    host, dev, err = _both_ways(args + ["--counts_out", "mine.counts", "--counts_only"], str(tmp_path), ["mine.counts"])
    assert host["mine.counts"] == dev["mine.counts"]


def test_many_blocks_small_batches(tmp_path):
    """Synthetic inputs that stress the device path: five chromosomes of four 30-Mb blocks, 8 % of the rows with age_begin = 0 (the F
    path; ranges from the first age bin over more than 64 bins), three targets x two references, 4-MB stream windows and batches of
    20 000 records (several submissions per hand-over)."""
    d = str(tmp_path)
    synth_files.write_inputs(d, chroms=("1", "2", "3", "4", "5"), snps_per_chr=20000, seed=11, span=110_000_000, extra_targets=2, extra_refs=1)
    pairs = [(f"{t}.colate.in", f"{r}.colate.in", f"out_{t}_{r}") for t in ("T", "T1", "T2") for r in ("R", "R1")]
    open(os.path.join(d, "pairs.txt"), "w").write("".join(" ".join(p) + "\n" for p in pairs))
    args = ["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "3", "--num_bootstraps", "3", "--pairs", "pairs.txt",
            "--counts_only"]
    outs = [p[2] + ".counts" for p in pairs]
    host, dev, err = _both_ways(args, d, outs, COLATE_UNIFORM_WINDOW_MB="4", COLATE_DEVICE_FILL_BATCH="20000")
    for o in outs:
        assert host[o] == dev[o], o
    m = re.search(r"age sampling on the GPU: (\d+) \(pair, block\) jobs", err)
    assert int(m.group(1)) >= 6 * 5 * 3  # (every pair, every chromosome, most blocks)


# ---- pairs the device hands back to the host (a flagged table, a block larger than a batch, more than 512 blocks): the host fills
# them again, and the .counts must still be the host's bytes.  Each case asserts the number of pairs handed back.
ARGS = ["--mode", "mut", "--mut", "P", "--chr", "chr.txt", "--bins", "3,7,0.2", "--seed", "5", "--num_bootstraps", "3", "--counts_only"]


def _pairs(d, pairs):
    open(os.path.join(d, "pairs.txt"), "w").write("".join(f"{t}.colate.in {r}.colate.in {o}\n" for t, r, o in pairs))
    return [o + ".counts" for _, _, o in pairs]


def _single(target):
    return ARGS + ["--target_tmp", f"{target}.colate.in", "--reference_tmp", "R.colate.in", "--counts_out", "one.counts", "-o", "one"]


def _same(host, dev):
    for o in host:
        assert host[o] == dev[o], o


def _beyond_grid_inputs(d):
    """Forty rows of chromosome 2 pushed beyond the age grid (non-F: every pair that uses one is flagged by the kernel); T1 has no
    record at those positions, so the pairs of T1 use none of them and stay on the device."""
    synth_files.write_inputs(d, chroms=("1", "2", "3"), snps_per_chr=3000, seed=21, extra_targets=1, extra_refs=1)
    pos = set(synth_files.push_beyond_the_age_grid(os.path.join(d, "P_chr2.mut"), 40))
    assert synth_files.keep_records(os.path.join(d, "T1.colate.in"), lambda c, bp: not (c == "2" and bp in pos)) > 0


def test_kernel_flag_hands_back_only_the_flagged_pairs(tmp_path):
    """A --pairs list with flagged and clean pairs side by side in the device's tables: the per-slot read-back takes the clean
    pairs' tables and hands the flagged ones back."""
    d = str(tmp_path)
    _beyond_grid_inputs(d)
    outs = _pairs(d, [("T", "R", "a"), ("T1", "R", "b"), ("T", "R1", "c"), ("T1", "R1", "d")])
    # (T, R) and (T, R1) use pushed rows; (T1, *) do not
    host, dev, err = _both_ways(ARGS + ["--pairs", "pairs.txt"], d, outs, redone=2, host_redone=2, COLATE_UNIFORM_WINDOW_MB="4")
    _same(host, dev)


@pytest.mark.parametrize("target,redone", [("T", 1), ("T1", 0)])
def test_kernel_flag_single_pair(target, redone, tmp_path):
    d = str(tmp_path)
    _beyond_grid_inputs(d)
    host, dev, err = _both_ways(_single(target), d, ["one.counts"], redone=redone, host_redone=redone)
    _same(host, dev)


def test_block_larger_than_a_batch_goes_to_the_host(tmp_path):
    """Batches of 1024 records: T's one-block chromosomes have more used SNPs than that (the hand-over gives the pair to the host),
    T1 keeps a tenth of its records (every block fits)."""
    d = str(tmp_path)
    synth_files.write_inputs(d, chroms=("1", "2"), snps_per_chr=6000, seed=22, span=25_000_000, extra_targets=1)
    assert synth_files.keep_records(os.path.join(d, "T1.colate.in"), lambda c, bp: bp % 10 == 0) > 0
    outs = _pairs(d, [("T", "R", "big"), ("T1", "R", "small")])
    host, dev, err = _both_ways(ARGS + ["--pairs", "pairs.txt"], d, outs, redone=1, host_redone=0, COLATE_DEVICE_FILL_BATCH="1024")
    _same(host, dev)


N_CONTIGS = 520  # (DeviceSampler::kMaxBlocks = 512 tables per pair on the device; every --chr entry closes a block)


def _many_contigs(d, empty_tail):
    """520 small contigs (a block each).  `empty_tail`: T1 has no record on contigs 513 on, so its blocks from 512 on have no used
    SNP -- and still exist."""
    synth_files.write_inputs(d, chroms=tuple(f"c{i}" for i in range(N_CONTIGS)), snps_per_chr=8, seed=23, span=20_000, extra_targets=1)
    if empty_tail:
        tail = {f"c{i}" for i in range(512, N_CONTIGS)}
        assert synth_files.keep_records(os.path.join(d, "T1.colate.in"), lambda c, bp: c not in tail) > 0


def test_more_than_512_blocks_with_used_tail(tmp_path):
    """(a) Both pairs have used SNPs in blocks 512 on: both are filled on the host."""
    d = str(tmp_path)
    _many_contigs(d, empty_tail=False)
    outs = _pairs(d, [("T1", "R", "x"), ("T", "R", "y")])
    host, dev, err = _both_ways(ARGS + ["--pairs", "pairs.txt"], d, outs, redone=2, host_redone=0)
    _same(host, dev)


def test_more_than_512_blocks_with_empty_tail(tmp_path):
    """(b) T1's blocks from 512 on hold no used SNP, and its pair is not in the last slot: its tables 512 on would be the next
    pair's.  It is filled on the host like the other."""
    d = str(tmp_path)
    _many_contigs(d, empty_tail=True)
    outs = _pairs(d, [("T1", "R", "x"), ("T", "R", "y")])
    host, dev, err = _both_ways(ARGS + ["--pairs", "pairs.txt"], d, outs, redone=2, host_redone=0)
    _same(host, dev)


def test_more_than_512_blocks_with_empty_tail_single_pair(tmp_path):
    """(c) The same pair through the single-pair CLI (its slot is the last: its tables 512 on would lie past the device's)."""
    d = str(tmp_path)
    _many_contigs(d, empty_tail=True)
    host, dev, err = _both_ways(_single("T1"), d, ["one.counts"], redone=1, host_redone=0)
    _same(host, dev)


def test_masked_pair_flagged_by_the_device_keeps_its_masks(tmp_path):
    """The masked fixture with rows beyond the age grid: the device flags the pair, and the host's sequential refill applies the
    masks -- the same bytes as the host engine and as the sequential feeder (COLATE_THREADS=1), which differ without them."""
    d = str(tmp_path)
    case = gl.l3_stage("l3_masks", d)
    synth_files.push_beyond_the_age_grid(os.path.join(d, "P_chr1.mut.gz"), 10)
    args = list(case["args"])
    args[args.index("-o") + 1] = "mine"
    args += ["--counts_out", "mine.counts", "--counts_only"]
    host, dev, err = _both_ways(args, d, ["mine.counts"], redone=1, host_redone=1)
    _same(host, dev)
    r = _run(args, d, COLATE_THREADS="1")
    assert r.returncode == 0, r.stderr.decode()[-800:]
    assert "pairs front end on" not in r.stderr.decode()
    assert open(os.path.join(d, "mine.counts"), "rb").read() == dev["mine.counts"]


_TOUCHED_CHILD = (
    "import ctypes, os, sys\n"
    "sys.path.insert(0, sys.argv[1])\n"
    "from colate_amd._lib import lib\n"
    "os.chdir(sys.argv[2])\n"
    "argv = [b'Colate'] + [a.encode() for a in sys.argv[3:]]\n"
    "rc = lib.colate_mut_main(len(argv), (ctypes.c_char_p * len(argv))(*argv))\n"
    "print('touched', lib.colate_device_touched(), flush=True)\n"
    "sys.exit(rc)\n"
)


@pytest.mark.parametrize("device_fill", [None, "0"])
def test_device_fill_marks_the_process_as_device_touched(tmp_path, device_fill):
    """`--pairs ... --counts_only` through colate_mut_main in a fresh process: the age sampling on the device brings up the HIP
    runtime, so the process is marked (colate_device_touched() = 1, what keeps a later --ranks from forking it); with
    COLATE_DEVICE_FILL=0 nothing in the run touches the device and the mark stays 0."""
    meta = gl.l3_pairs_stage(str(tmp_path))
    args = ["--mode", "mut", "--mut", "P"] + meta["common_args"] + ["--pairs", "pairs.txt", "--counts_only"]
    env = dict(os.environ, COLATE_TIMING="1")
    env.pop("COLATE_DEVICE_FILL", None)
    if device_fill is not None:
        env["COLATE_DEVICE_FILL"] = device_fill
    r = subprocess.run([os.sys.executable, "-c", _TOUCHED_CHILD, ROOT, str(tmp_path)] + args, capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-1500:])
    if device_fill is None:
        assert "age sampling on the GPU:" in r.stderr and "touched 1" in r.stdout, (r.stdout, r.stderr[-1500:])
    else:
        assert "age sampling on the host (COLATE_DEVICE_FILL=0)" in r.stderr and "touched 0" in r.stdout, (r.stdout, r.stderr[-1500:])
