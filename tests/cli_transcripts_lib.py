"""What `Colate` says and writes, command line by command line (TEST INFRASTRUCTURE): tiny inputs written with the generators the
suite already has, the command lines of every list mode, single run, cursor fallback and refusal, and the runner that returns a
transcript -- exit code, stdout and stderr -- without the lines that carry times.  tests/golden/cli_transcripts/ holds the
transcripts of the commit before the drivers were folded into one list front end and one per-pair back end (`python
tests/cli_transcripts_lib.py record BINARY DIR host|device` writes them from any binary): the drivers may move, their words may not."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cli_transcripts")
CLI = os.path.join(os.path.dirname(HERE), "colate_amd", "bin", "Colate")

FIT = ["--num_bootstraps", "2", "--seed", "5"]
IVL_FIT = FIT + ["--max_iter", "60", "--min_iter", "20"]  # (the host twin of the interval-dated fit is slow: a short fit)
BINS = ["--bins", "3,7,0.2"]
MUT = ["--mut", "P", "--chr", "chr.txt"]
NO_FILL = {"COLATE_DEVICE_FILL": "0"}
IVL, CMP, TOPO = {"COLATE_DEVICE_INTERVAL": "0"}, {"COLATE_DEVICE_COMPARE": "0"}, {"COLATE_DEVICE_TOPO": "0"}
NO_INDEX = {"COLATE_INDEXED_WALK": "0"}


# ------------------------------------------------------------------ the inputs
def stage(d):
    """the inputs of every command line under d, one directory per generator: pairs/ (synth_files through interval_groups_lib: T, T1,
    T2 x R, R1, the mask tm, warm.coal with another number of epochs than BINS), l3/ (tests/golden/l3_pairs), cmp/ and cmp_desc/ (rows
    that descend), topo/ and topo_big/ (counts beyond 16 bits)"""
    import compare_tmp_lib as cl
    import count_topo_lib as tl
    import fill_samples_lib as fs
    import golden_lib
    import interval_groups_lib as gl
    import interval_walk_lib as wl

    d = str(d)
    p = os.path.join(d, "pairs")
    os.makedirs(p)
    gl.cli_inputs(_Path(p), snps_per_chr=400)
    _write(p, "mut_pairs.txt", ["T.colate.in R.colate.in mut_pairs_p1",
                                "T1.colate.in R.colate.in mut_pairs_p2 500 0",             # two ages
                                "T2.colate.in R1.colate.in mut_pairs_p3 coal=warm.coal",   # another number of epochs: a second class
                                "T.colate.in R1.colate.in mut_pairs_p4 7000 target_mask=tm"])
    _write(p, "ivl_pairs.txt", [" ".join([t, r, "mut_interval_pairs_" + out] + extra) for t, r, out, extra, _ in gl.SIX_PAIRS])
    _write(p, "samples.txt", wl.SAMPLES)
    golden_lib.l3_pairs_stage(os.path.join(d, "l3"))
    _write(os.path.join(d, "l3"), "samples.txt", fs.sample_lines(fs.L3_LISTS[0][0]))
    for sub, write, kw in (("cmp", cl.write_file_case, {}), ("cmp_desc", cl.write_file_case, {}), ("topo", tl.write_file_case, {}),
                           ("topo_big", tl.write_file_case, {"big_counts": True})):
        os.makedirs(os.path.join(d, sub))
        write(os.path.join(d, sub), **kw)
    path = os.path.join(d, "cmp_desc", "P_chr2.mut")
    lines = open(path).read().split("\n")
    lines[40], lines[200] = lines[200], lines[40]
    open(path, "w").write("\n".join(lines))
    return d


class _Path(str):
    """(interval_groups_lib.cli_inputs joins with `/`)"""

    def __truediv__(self, other):
        return _Path(os.path.join(self, other))


def _write(d, name, lines):
    with open(os.path.join(d, name), "w") as f:
        f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------ the command lines
class Line:
    """name; the directory of stage() it runs in; the arguments; what the host run adds to them and sets"""

    def __init__(self, name, sub, args, host_env, host_args=()):
        self.name, self.sub, self.args, self.host_env, self.host_args = name, sub, list(args), dict(host_env), list(host_args)


COUNTS_ONLY = ["--counts_only"]
LIST_MODES = [
    Line("mut_pairs", "pairs", ["--mode", "mut", "--pairs", "mut_pairs.txt"] + MUT + BINS + FIT, NO_FILL, COUNTS_ONLY),
    Line("mut_samples", "l3", ["--mode", "mut", "--samples", "samples.txt", "-o", "mut_samples"] + MUT + BINS + FIT, NO_FILL, COUNTS_ONLY),
    Line("mut_interval_pairs", "pairs", ["--mode", "mut_interval", "--pairs", "ivl_pairs.txt"] + MUT + BINS + IVL_FIT, IVL),
    Line("mut_interval_samples", "pairs", ["--mode", "mut_interval", "--samples", "samples.txt", "-o", "mut_interval_samples"] + MUT + BINS + IVL_FIT, IVL),
    Line("compare_tmp_samples", "cmp", ["--mode", "compare_tmp", "--samples", "samples.txt", "-o", "compare_tmp_samples"] + MUT, CMP),
    Line("count_topo_samples", "topo", ["--mode", "count_topo", "--samples", "samples.txt", "-o", "count_topo_samples", "--seed", "5"] + MUT, TOPO),
    Line("count_topo_profile", "topo", ["--mode", "count_topo", "--samples", "samples.txt", "-o", "count_topo_profile", "--seed", "5",
                                        "--age_profile", "1,4,0.5", "--profile_only"] + MUT, TOPO),
]
PAIR = ["--target_tmp", "T1.colate.in", "--reference_tmp", "R.colate.in"]
SINGLE_RUNS = [
    Line("mut_single", "l3", ["--mode", "mut", "-o", "mut_single", "--target_age", "500"] + PAIR + MUT + BINS + FIT, NO_FILL, COUNTS_ONLY),
    Line("mut_interval_single", "pairs", ["--mode", "mut_interval", "-o", "mut_interval_single", "--target_mask", "tm"] + PAIR + MUT + BINS + IVL_FIT, IVL),
    Line("compare_tmp_single", "cmp", ["--mode", "compare_tmp", "--target_tmp", "s0.colate.in", "--reference_tmp", "s2.colate.in",
                                       "-o", "compare_tmp_single.txt"] + MUT, CMP),
    Line("count_topo_single", "topo", ["--mode", "count_topo", "-i", "s3.colate.in", "--target_tmp", "s0.colate.in", "--reference_tmp", "s1.colate.in",
                                       "-o", "count_topo_single.txt", "--seed", "5"] + MUT, TOPO),
]
CURSOR_FALLBACKS = [  # (host runs only)
    Line("count_topo_cursors", "topo_big", LIST_MODES[5].args, TOPO),
    Line("compare_tmp_cursors", "cmp_desc", LIST_MODES[4].args, CMP),
    Line("mut_interval_cursors", "pairs", LIST_MODES[3].args, dict(IVL, **NO_INDEX)),
]
UNWRITABLE = [  # (host runs only) the first per-pair file cannot be written: one error line, exit 1, nothing said about the list file
    Line("compare_tmp_unwritable", "cmp", ["--mode", "compare_tmp", "--samples", "samples.txt", "-o", "nodir/o"] + MUT, CMP),
    Line("count_topo_unwritable", "topo", ["--mode", "count_topo", "--samples", "samples.txt", "-o", "nodir/o", "--age_profile", "1,4,0.5"] + MUT, TOPO),
]
DEVICE_LINES = LIST_MODES + SINGLE_RUNS
HOST_LINES = DEVICE_LINES + CURSOR_FALLBACKS

# Per list mode: the options it refuses (the lists of the drivers), those it wants per line, and a line that lacks a needed argument.
REFUSALS = {
    "mut_pairs": (["--mode", "mut", "--pairs", "mut_pairs.txt"], [], ["target_mask", "reference_mask", "coal"], BINS),
    "mut_samples": (["--mode", "mut", "--samples", "samples.txt"],
                    ["pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "ranks"], [], MUT + BINS),
    "mut_interval_pairs": (["--mode", "mut_interval", "--pairs", "ivl_pairs.txt"],
                           ["target_tmp", "reference_tmp", "rows", "write_rows", "output", "ranks", "target_age", "reference_age"],
                           ["target_mask", "reference_mask", "coal"], BINS),
    "mut_interval_samples": (["--mode", "mut_interval", "--samples", "samples.txt"],
                             ["pairs", "rows", "target_tmp", "reference_tmp", "write_rows", "target_mask", "reference_mask", "ranks", "target_age",
                              "reference_age"], [], MUT + BINS),
    "compare_tmp_samples": (["--mode", "compare_tmp", "--samples", "samples.txt"],
                            ["pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "bins", "coal",
                             "num_bootstraps", "ranks", "devices"], [], MUT),
    "count_topo_samples": (["--mode", "count_topo", "--samples", "samples.txt"],
                           ["input", "pairs", "target_tmp", "reference_tmp", "target_mask", "reference_mask", "target_age", "reference_age", "bins",
                            "coal", "num_bootstraps", "ranks", "devices"], [], MUT),
}


def refusal_lines(mode):
    """(label, arguments) of every refusal of a list mode: one per refused option -- the mode's list first, then the per-line form --
    and the line without a needed argument"""
    head, refused, per_line, incomplete = REFUSALS[mode]
    out = [("--" + o, head + MUT + ["--" + o, "2"]) for o in refused + per_line]
    return out + [("incomplete", head + incomplete)]


# ------------------------------------------------------------------ the runner
def run(binary, cwd, args, env=None, timeout=120):
    """`binary ARGS` in cwd with no COLATE_* variable but those of env: (exit code, transcript)"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("COLATE_")}
    e.update(env or {})
    r = subprocess.run([binary] + list(args), cwd=str(cwd), capture_output=True, text=True, env=e, timeout=timeout)
    keep = lambda text: "".join(x + "\n" for x in text.splitlines() if not x.startswith(("CPU Time spent: ", "Timing:")))
    return r.returncode, f"exit {r.returncode}\n---- stdout\n{keep(r.stdout)}---- stderr\n{keep(r.stderr)}"


def run_line(binary, d, line, host):
    """the line in its directory under d, on the host path or with nothing set"""
    return run(binary, os.path.join(str(d), line.sub), line.args + (line.host_args if host else []), line.host_env if host else None)


def run_refusals(binary, d, mode):
    """the refusals of a mode, one after the other, as one transcript"""
    sub = {l.name: l.sub for l in LIST_MODES}[mode]
    return "".join(f"==== {label}\n" + run(binary, os.path.join(str(d), sub), args)[1] for label, args in refusal_lines(mode))


def golden(name, kind):
    with open(os.path.join(GOLDEN, f"{name}.{kind}.txt")) as f:
        return f.read()


def files_of(d):
    """{path below d: bytes} of every file"""
    out = {}
    for root, _, names in os.walk(str(d)):
        for n in names:
            with open(os.path.join(root, n), "rb") as f:
                out[os.path.relpath(os.path.join(root, n), str(d))] = f.read()
    return out


def record(binary, out_dir, kind, work):
    """the transcripts of `binary` as files under out_dir: kind `host` (every line on the host path, and the refusals) or `device`"""
    os.makedirs(out_dir, exist_ok=True)
    stage(os.path.join(work, "in"))
    texts = {}
    for line in (HOST_LINES + UNWRITABLE if kind == "host" else DEVICE_LINES):
        texts[line.name] = run_line(binary, os.path.join(work, "in"), line, kind == "host")[1]
    if kind == "host":
        for mode in REFUSALS:
            texts["refusals_" + mode] = run_refusals(binary, os.path.join(work, "in"), mode)
    for name, text in texts.items():
        with open(os.path.join(out_dir, f"{name}.{kind}.txt"), "w") as f:
            f.write(text)
    return sorted(texts)


if __name__ == "__main__":
    import tempfile

    sys.path.insert(0, os.path.dirname(HERE))
    _, _, binary, out_dir, kind = sys.argv
    with tempfile.TemporaryDirectory() as work:
        print("\n".join(record(os.path.abspath(binary), out_dir, kind, work)))
