"""Shared by the CoalRate tests (TEST INFRASTRUCTURE): the committed fixtures (tests/golden/coalrate_*, written by
tests/golden/make_golden_coalrate.py), the CLI runner, the token rule of the comparison with the reference's .coal, and
random inputs for the accumulator checks."""
import json
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "colate_amd", "bin", "CoalRate")
SHAPE_KEYS = ("launches", "cpw_min", "cpw_max", "lanes_per_call", "lds")   # of colate_amd.coalrate[_tree]_launch_shape()
CASES = sorted(d[len("coalrate_"):] for d in os.listdir(GOLDEN) if d.startswith("coalrate_")
               and os.path.isdir(os.path.join(GOLDEN, d)))


def case_dir(name):
    return os.path.join(GOLDEN, f"coalrate_{name}")


def cli_env(device, extra_env=None):
    env = dict(os.environ)
    env.pop("COLATE_DEVICE_COALRATE", None)
    if not device:
        env["COLATE_DEVICE_COALRATE"] = "0"
    env.update(extra_env or {})
    return env


def run_cli(args, cwd, device, timeout=600, extra_env=None):
    return subprocess.run([CLI] + list(args), cwd=cwd, capture_output=True, text=True, env=cli_env(device, extra_env),
                          timeout=timeout)


def run_case(name, out_prefix, device, timeout=600, extra_env=None):
    """Runs the CLI on a fixture (inputs read in place, OUT.coal written at out_prefix)."""
    d = case_dir(name)
    with open(os.path.join(d, "case.json")) as f:
        args = json.load(f)["args"]
    args = list(args)
    args[args.index("-o") + 1] = out_prefix
    return run_cli(args, d, device, timeout, extra_env)


def sixth_digit_unit(token):
    """One unit in the sixth significant digit of a number printed with 6 significant digits."""
    x = abs(float(token))
    return 10.0 ** (math.floor(math.log10(x)) - 5)


def compare_coal(ours_path, ref_path):
    """The label row, the epoch row and the `i j` tokens identical; non-finite and zero rate tokens identical as text;
    every finite rate token identical or at most one unit in its sixth significant digit away.  Returns (tokens compared,
    tokens not identical); raises AssertionError otherwise."""
    with open(ours_path) as f:
        A = f.read().split("\n")
    with open(ref_path) as f:
        B = f.read().split("\n")
    assert len(A) == len(B), (len(A), len(B))
    assert A[0] == B[0], (A[0], B[0])
    assert A[1] == B[1], (A[1], B[1])
    total = differ = 0
    for a, b in zip(A[2:], B[2:]):
        ta, tb = a.split(" "), b.split(" ")
        assert len(ta) == len(tb), (a, b)
        assert ta[:2] == tb[:2], (a, b)
        for x, y in zip(ta[2:], tb[2:]):
            total += 1
            if x == y:
                continue
            differ += 1
            fx, fy = float(x), float(y)  # (an empty trailing token is identical or an error above)
            assert math.isfinite(fx) and math.isfinite(fy) and fx != 0.0 and fy != 0.0, (x, y, a, b)
            assert abs(fx - fy) <= 1.0000001 * max(sixth_digit_unit(x), sixth_digit_unit(y)), (x, y, a, b)
    return total, differ


def bins_epochs(lower, upper, step, years_per_gen=28.0):
    """coal.cpp:267-325 in double (the fields through float32, as stof reads them)."""
    lower, upper, step = (float(np.float32(v)) for v in (lower, upper, step))
    ep = [0.0]
    b = lower
    log10 = math.log(10)
    while b < upper:
        ep.append(math.exp(log10 * b) / years_per_gen)
        b += step
    ep.append(math.exp(log10 * upper) / years_per_gen)
    ep.append(max(1e8, 10 * ep[-1]) / years_per_gen)
    return np.array(ep)


def random_tree(rng, N, ages=None, Ne=2000.0):
    """parent[2N-1] and branch lengths (Relate labelling, root 2N-2): a random coalescent topology whose coalescences all
    lie above the oldest sample age."""
    nn = 2 * N - 1
    parent = np.full(nn, -1, dtype=np.int32)
    h = np.zeros(nn)
    if ages is not None:
        h[:N] = ages
    t = float(h.max())
    active = list(range(N))
    for label in range(N, nn):
        k = len(active)
        t += rng.exponential(2.0 * Ne / (k * (k - 1) / 2.0))
        i = int(rng.integers(k))
        a = active.pop(i)
        j = int(rng.integers(k - 1))
        b = active.pop(j)
        parent[a] = parent[b] = label
        h[label] = t
        active.append(label)
    bl = np.where(parent >= 0, h[np.maximum(parent, 0)] - h, 0.0)
    return parent, bl


def random_input(rng, N, T, G, S, num_blocks, ancient, epochs):
    """Trees, weights, blocks (a few changes, not at chunk boundaries only), group vectors and ages for the accumulators."""
    ages = None
    if ancient:
        ages = np.zeros(N)
        idx = rng.choice(N, size=max(1, N // 4), replace=False)
        ages[idx] = np.round(rng.uniform(1.0, 0.9 * epochs[3], size=idx.size), 2)
    parents = np.zeros((T, 2 * N - 1), dtype=np.int32)
    bl = np.zeros((T, 2 * N - 1))
    for t in range(T):
        parents[t], bl[t] = random_tree(rng, N, ages)
    weights = np.round(rng.uniform(0.5, 9000.0, T), 3)
    blocks = np.sort(rng.integers(0, num_blocks, T)).astype(np.int32)
    gv = rng.integers(0, S, T).astype(np.int32)
    groups = rng.integers(0, G, (S, N)).astype(np.int32)
    return parents, bl, weights, blocks, gv, groups, ages


# 36 calls in nine blocks whose boundaries fall inside the chunks of four: chunk c ends in block min(c + 1, 8)
GROW_BLOCKS = np.minimum((np.arange(36) + 2) // 4, 8).astype(np.int32)


def sum_reallocations(blocks, cap):
    """The capacity rule of the device walkers' per-block sums over chunks of `cap` calls (capacity 0 at first; a chunk
    needs its largest block + 1; a larger need takes max(need, 2 * capacity)): (reallocations, those among them that copy
    blocks which earlier chunks have added to)."""
    capacity, reallocations, copying, seen = 0, 0, 0, False
    for i in range(0, len(blocks), cap):
        need = int(blocks[i:i + cap].max()) + 1
        if need > capacity:
            capacity = max(need, 2 * capacity)
            reallocations += 1
            copying += seen
        seen = True
    return reallocations, copying


def accumulate_in_child(tmp_path, inp, epochs, device, timeout, chunk_trees=None, with_shape=False):
    """coalrate_accumulate in a child process under its own time limit; inp = random_input's tuple plus (num_blocks, G).
    Returns (num, denom), with_shape: and colate_amd.coalrate_launch_shape() after the call; raises on a child that fails
    (nothing is retried)."""
    import sys
    parents, bl, weights, blocks, gv, groups, ages, num_blocks, G = inp
    src = os.path.join(str(tmp_path), "coalrate_in.npz")
    dst = os.path.join(str(tmp_path), f"coalrate_out_{int(device)}.npz")
    np.savez(src, parents=parents, bl=bl, weights=weights, blocks=blocks, gv=gv, groups=groups,
             ages=np.zeros(0) if ages is None else ages, num_blocks=num_blocks, G=G, epochs=epochs)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("COLATE_COALRATE_CHUNK_TREES", None)
    if chunk_trees:
        env["COLATE_COALRATE_CHUNK_TREES"] = str(chunk_trees)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), src, dst, str(int(device))], capture_output=True, text=True,
                       env=env, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.load(dst)
    if with_shape:
        return out["num"], out["den"], dict(zip(SHAPE_KEYS, out["shape"].tolist()))
    return out["num"], out["den"]


if __name__ == "__main__":
    import sys
    import colate_amd
    z = np.load(sys.argv[1])
    ages = z["ages"] if z["ages"].size else None
    num, den = colate_amd.coalrate_accumulate(z["parents"], z["bl"], z["weights"], z["blocks"], int(z["num_blocks"]), z["gv"],
                                              z["groups"], int(z["G"]), z["epochs"], ages, device=bool(int(sys.argv[3])))
    np.savez(sys.argv[2], num=num, den=den, shape=[colate_amd.coalrate_launch_shape()[k] for k in SHAPE_KEYS])
