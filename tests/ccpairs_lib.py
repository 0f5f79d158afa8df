"""Shared by the CondCoalRates --pairs tests (TEST INFRASTRUCTURE): the committed fixtures (tests/golden/ccpairs_*, written
by golden/make_golden_ccpairs.py), the CLI runners, every ordered group pair of an input, and the accumulators of a pair list
next to those of its single pairs in a child process (the GPU steps of the tests)."""
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np

import condcoal_lib as cl

GOLDEN = cl.GOLDEN
CLI = cl.CLI
CASES = sorted(d[len("ccpairs_"):] for d in os.listdir(GOLDEN) if d.startswith("ccpairs_")
               and os.path.isdir(os.path.join(GOLDEN, d)))


def case_dir(name):
    return os.path.join(GOLDEN, f"ccpairs_{name}")


def case_args(name):
    with open(os.path.join(case_dir(name), "case.json")) as f:
        return json.load(f)["args"]


def case_pairs(name):
    """[(groups token, expected table file)] of a fixture's pairs.txt."""
    with open(os.path.join(case_dir(name), "pairs.txt")) as f:
        return [tuple(line.split()) for line in f if line.strip()]


def env_for(device, **extra):
    env = dict(os.environ, **extra)
    if not device:
        env["COLATE_DEVICE_CONDCOAL"] = "0"
    else:
        env.pop("COLATE_DEVICE_CONDCOAL", None)
    return env


def run(cwd, args, device, timeout=600, **extra_env):
    return subprocess.run([CLI] + list(args), cwd=str(cwd), capture_output=True, text=True, env=env_for(device, **extra_env),
                          timeout=timeout)


def copy_dir(src, dst):
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), str(dst))


def groups_of(poplabels):
    with open(poplabels) as f:
        return sorted({line.split()[1] for line in f.read().splitlines()[1:] if line.strip()})


def strip_single(args):
    """A single run's arguments without --groups / --output (and its value)."""
    out, skip = [], False
    for a in args:
        if skip:
            skip = False
            continue
        if a in ("--groups", "--output", "-o"):
            skip = True
            continue
        out.append(a)
    return out


def write_list(path, pairs):
    """pairs: [(groups token, output)]."""
    with open(path, "w") as f:
        f.write("".join(f"{g} {o}\n" for g, o in pairs))


def pairs_vs_singles(tmp_path, shared_args, groups_tokens, device, timeout=600, **extra_env):
    """Runs the CLI once with --pairs and once per pair alone in tmp_path (the inputs are there); returns the list of
    (groups token, pairs output, single output) file paths."""
    pairs = [(g, f"p{k}.txt") for k, g in enumerate(groups_tokens)]
    write_list(os.path.join(str(tmp_path), "list.txt"), pairs)
    r = run(tmp_path, shared_args + ["--pairs", "list.txt"], device, timeout, **extra_env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = []
    for k, (g, o) in enumerate(pairs):
        s = f"s{k}.txt"
        r = run(tmp_path, shared_args + ["--groups", g, "-o", s], device, timeout)
        assert r.returncode == 0, (g, r.stderr[-3000:])
        res.append((g, os.path.join(str(tmp_path), o), os.path.join(str(tmp_path), s)))
    return res


def members(group_of_hap, g):
    return np.flatnonzero(np.asarray(group_of_hap) == g).astype(np.int32) if g >= 0 else np.zeros(0, dtype=np.int32)


def accumulate_pairs_and_singles(inp, focal_group, cond_group, epochs, efocal, device, singles=True):
    """condcoal_accumulate_pairs, and condcoal_accumulate of every pair alone (singles=True): (num, denom, [(num, denom)])."""
    import colate_amd

    kw = {k: inp[k] for k in ("parents", "branch_lengths", "factors", "blocks", "num_blocks", "group_of_hap", "num_groups",
                              "sample_ages")}
    num, den = colate_amd.condcoal_accumulate_pairs(focal_group=focal_group, cond_group=cond_group, epochs=epochs,
                                                    epochs_focal=efocal, device=device, **kw)
    one = []
    if singles:
        for fg, cg in zip(focal_group, cond_group):
            one.append(colate_amd.condcoal_accumulate(focal=members(inp["group_of_hap"], fg),
                                                      cond=members(inp["group_of_hap"], cg), epochs=epochs,
                                                      epochs_focal=efocal, device=device, **kw))
    return num, den, one


def in_child(tmpdir, inp, focal_group, cond_group, epochs, efocal, device, timeout, singles=True, env=None):
    """accumulate_pairs_and_singles in a child process under a time limit: (num, denom, single_num, single_denom) with the
    singles stacked [P, ...] (None without singles)."""
    tag = f"{os.getpid()}_{random.getrandbits(32)}"
    src = os.path.join(str(tmpdir), f"pin_{tag}.npz")
    dst = os.path.join(str(tmpdir), f"pout_{tag}.npz")
    arrays = {k: np.asarray(v) for k, v in inp.items() if v is not None}
    np.savez(src, epochs=epochs, efocal=efocal, focal_group=np.asarray(focal_group), cond_group=np.asarray(cond_group),
             **arrays)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), src, dst, "1" if device else "0", "1" if singles else "0"],
                       capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = np.load(dst)
    if singles:
        return out["num"], out["denom"], out["snum"], out["sden"]
    return out["num"], out["denom"], None, None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


if __name__ == "__main__":  # the child of in_child
    sys.path.insert(0, cl.ROOT)
    z = np.load(sys.argv[1])
    inp = {k: z[k] for k in ("parents", "branch_lengths", "factors", "blocks", "group_of_hap", "focal", "cond")}
    inp["num_blocks"] = int(z["num_blocks"])
    inp["num_groups"] = int(z["num_groups"])
    inp["sample_ages"] = z["sample_ages"] if "sample_ages" in z.files else None
    num, den, one = accumulate_pairs_and_singles(inp, z["focal_group"], z["cond_group"], z["epochs"], z["efocal"],
                                                 sys.argv[3] == "1", sys.argv[4] == "1")
    extra = {}
    if one:
        extra = dict(snum=np.stack([a for a, _ in one]), sden=np.stack([b for _, b in one]))
    np.savez(sys.argv[2], num=num, denom=den, **extra)
