"""Shared by the `CoalRate --mode tree` tests (TEST INFRASTRUCTURE): the committed fixtures (tests/golden/crtree_*, written
by tests/golden/make_golden_coalrate_tree.py), their runner, and random inputs for the accumulator checks: trees with
quantised heights (ties among internal nodes and with sample ages) and epochs that node times hit exactly."""
import json
import os
import subprocess
import sys

import numpy as np

import coalrate_lib as cl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CASES = sorted(d[len("crtree_"):] for d in os.listdir(GOLDEN) if d.startswith("crtree_")
               and os.path.isdir(os.path.join(GOLDEN, d)))
EXPECTED_CASES = ["ancient", "blocks", "chr", "modern", "settings", "ties"]

LDS_KEYS = 16384          # coalrate_tree.h kLdsKeys: padded keys up to which the device sorts in LDS (N <= 8192)
TIE_EPOCHS = np.array([0.0, 64.0, 128.0, 1024.0, 1e7])   # multiples of the quantum: node times equal boundaries


def padded_keys(N):
    P = 4
    while P < 2 * N - 1:
        P *= 2
    return P


def chunk_straddles_blocks(blocks, cap):
    """Whether some chunk of `cap` consecutive calls holds two block ids."""
    return any(len(set(blocks[i:i + cap].tolist())) > 1 for i in range(0, len(blocks), cap))


def case_dir(name):
    return os.path.join(GOLDEN, f"crtree_{name}")


def run_case(name, out_prefix, device, timeout=600, extra_env=None, cli=None):
    """Runs the CLI on a fixture (inputs read in place, OUT.coal written at out_prefix)."""
    d = case_dir(name)
    with open(os.path.join(d, "case.json")) as f:
        args = list(json.load(f)["args"])
    args[args.index("-o") + 1] = out_prefix
    if cli is None:
        return cl.run_cli(args, d, device, timeout, extra_env)
    return subprocess.run([cli] + args, cwd=d, capture_output=True, text=True, env=cl.cli_env(device, extra_env), timeout=timeout)


def quantised_tree(rng, N, ages=None, quantum=64.0):
    """parent[2N-1] and branch lengths; coalescences in label order at multiples of `quantum`, a third of the steps 0."""
    nn = 2 * N - 1
    h = np.zeros(nn)
    if ages is not None:
        h[:N] = ages
    parent = np.full(nn, -1, dtype=np.int32)
    waiting = sorted(range(N), key=lambda i: (h[i], i))
    active = []
    t = 0.0
    for label in range(N, nn):
        t += quantum * int(rng.integers(0, 3))
        while True:
            while waiting and h[waiting[0]] <= t:
                active.append(waiting.pop(0))
            if len(active) >= 2:
                break
            t += quantum
        i = int(rng.integers(len(active)))
        a = active.pop(i)
        j = int(rng.integers(len(active)))
        b = active.pop(j)
        parent[a] = parent[b] = label
        h[label] = t
        active.append(label)
    bl = np.where(parent >= 0, h[np.maximum(parent, 0)] - h, 0.0)
    return parent, bl


def random_input(rng, N, T, num_blocks, ancient, epochs, quantum=None, Ne=2000.0):
    """(parents, bl, weights, blocks, ages): blocks sorted with a few changes; quantum: quantised_tree with ages that are
    multiples of it; otherwise coalrate_lib.random_tree."""
    ages = None
    if ancient:
        ages = np.zeros(N)
        idx = rng.choice(N, size=max(1, N // 4), replace=False)
        if quantum:
            ages[idx] = quantum * rng.integers(1, 4, size=idx.size)
        else:
            ages[idx] = np.round(rng.uniform(1.0, 0.9 * epochs[3], size=idx.size), 2)
    parents = np.zeros((T, 2 * N - 1), dtype=np.int32)
    bl = np.zeros((T, 2 * N - 1))
    for t in range(T):
        parents[t], bl[t] = quantised_tree(rng, N, ages, quantum) if quantum else cl.random_tree(rng, N, ages, Ne)
    weights = np.round(rng.uniform(0.5, 9000.0, T), 3)
    blocks = np.sort(rng.integers(0, num_blocks, T)).astype(np.int32)
    return parents, bl, weights, blocks, ages


def accumulate_in_child(tmp_path, inp, num_blocks, epochs, device, timeout, chunk_trees=None, with_shape=False):
    """coalrate_tree_accumulate in a child process under its own time limit; inp = random_input's tuple.  Returns
    (num, denom), with_shape: and colate_amd.coalrate_tree_launch_shape() after the call; raises on a child that fails (nothing
    is retried)."""
    parents, bl, weights, blocks, ages = inp
    src = os.path.join(str(tmp_path), "crtree_in.npz")
    dst = os.path.join(str(tmp_path), f"crtree_out_{int(device)}.npz")
    if not os.path.exists(src):
        np.savez(src, parents=parents, bl=bl, weights=weights, blocks=blocks, ages=np.zeros(0) if ages is None else ages,
                 num_blocks=num_blocks, epochs=epochs)
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
        return out["num"], out["den"], dict(zip(cl.SHAPE_KEYS, out["shape"].tolist()))
    return out["num"], out["den"]


if __name__ == "__main__":
    import colate_amd
    z = np.load(sys.argv[1])
    ages = z["ages"] if z["ages"].size else None
    num, den = colate_amd.coalrate_tree_accumulate(z["parents"], z["bl"], z["weights"], z["blocks"], int(z["num_blocks"]),
                                                   z["epochs"], ages, device=bool(int(sys.argv[3])))
    np.savez(sys.argv[2], num=num, den=den, shape=[colate_amd.coalrate_tree_launch_shape()[k] for k in cl.SHAPE_KEYS])
