"""Shared by the CondCoalRates tests (TEST INFRASTRUCTURE): the committed fixtures, the CLI runner, the token rules of the
comparison with the reference's table, and fast random trees for the accumulator checks."""
import json
import math
import os
import random
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")
CASES = sorted(d[len("condcoal_"):] for d in os.listdir(GOLDEN) if d.startswith("condcoal_")
               and os.path.isdir(os.path.join(GOLDEN, d)))


def case_dir(name):
    return os.path.join(GOLDEN, f"condcoal_{name}")


def run_case(name, out_path, device, timeout=600, extra=()):
    """Runs the CLI on a fixture (inputs read in place, the table written to out_path)."""
    d = case_dir(name)
    with open(os.path.join(d, "case.json")) as f:
        args = json.load(f)["args"]
    args = [out_path if a == "out.txt" else a for a in args] + list(extra)
    env = dict(os.environ)
    if not device:
        env["COLATE_DEVICE_CONDCOAL"] = "0"
    else:
        env.pop("COLATE_DEVICE_CONDCOAL", None)
    return subprocess.run([CLI] + args, cwd=d, capture_output=True, text=True, env=env, timeout=timeout)


def compare_tables(ours_path, ref_path, rel_tol=1e-4):
    """Header and the boot / lineage_epoch / epoch.start / group tokens identical, non-finite and zero rates identical,
    finite rates within rel_tol.  Returns the largest relative difference; raises AssertionError otherwise."""
    with open(ours_path) as f:
        A = f.read().splitlines()
    with open(ref_path) as f:
        B = f.read().splitlines()
    assert len(A) == len(B), (len(A), len(B))
    assert A[0] == B[0]
    worst = 0.0
    for a, b in zip(A[1:], B[1:]):
        ta, tb = a.split(), b.split()
        assert ta[:4] == tb[:4], (a, b)
        x, y = float(ta[4]), float(tb[4])
        if not math.isfinite(y) or y == 0.0 or not math.isfinite(x) or x == 0.0:
            assert ta[4] == tb[4], (a, b)
            continue
        worst = max(worst, abs(x - y) / abs(y))
    assert worst <= rel_tol, worst
    return worst


def random_tree(rnd, N, Ne=5000.0, age_offset=0.0):
    """parent[2N-1], heights (Relate labelling, root 2N-2): a random coalescent topology, internal heights shifted by
    age_offset (above every sample age)."""
    parent = np.full(2 * N - 1, -1, dtype=np.int32)
    heights = np.zeros(2 * N - 1)
    active = list(range(N))
    t = 0.0
    for label in range(N, 2 * N - 1):
        k = len(active)
        t += rnd.expovariate(k * (k - 1) / 2.0 / (2.0 * Ne))
        i = rnd.randrange(k)
        a = active[i]
        active[i] = active[-1]
        active.pop()
        j = rnd.randrange(k - 1)
        b = active[j]
        active[j] = active[-1]
        active.pop()
        parent[a] = parent[b] = label
        heights[label] = t + age_offset
        active.append(label)
    return parent, heights


def caterpillar(rnd, N, age_offset=0.0, step=40.0):
    perm = list(range(N))
    rnd.shuffle(perm)
    parent = np.full(2 * N - 1, -1, dtype=np.int32)
    heights = np.zeros(2 * N - 1)
    prev, h = perm[0], age_offset
    for i in range(1, N):
        h += step * (0.5 + rnd.random())
        node = N + i - 1
        parent[prev] = parent[perm[i]] = node
        heights[node] = h
        prev = node
    return parent, heights


def branch_lengths(parent, heights, ages=None):
    h = heights.copy()
    if ages is not None:
        h[:len(ages)] = ages
    bl = np.zeros(len(parent))
    m = parent >= 0
    bl[m] = h[parent[m]] - h[m]
    return np.round(bl, 5)


def random_input(seed, N, T, G, ancient=False, n_focal=None, n_cond=None, caterpillar_at=None, num_blocks=3):
    """Trees, weights, blocks and groups for colate_amd.condcoal_accumulate."""
    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    ages = None
    offset = 0.0
    if ancient:
        ages = np.zeros(N)
        idx = rng.choice(N, size=max(1, N // 3), replace=False)
        ages[idx] = np.round(rng.uniform(50, 3000, size=idx.size), 1)
        offset = 3000.0
    parents = np.zeros((T, 2 * N - 1), dtype=np.int32)
    bls = np.zeros((T, 2 * N - 1))
    for t in range(T):
        p, h = caterpillar(rnd, N, offset) if t == caterpillar_at else random_tree(rnd, N, age_offset=offset)
        parents[t] = p
        bls[t] = branch_lengths(p, h, ages)
    factors = rng.uniform(100, 5e5, size=T).astype(np.float32)
    factors[-1] = -1.0
    blocks = np.sort(rng.integers(0, num_blocks, size=T)).astype(np.int32)
    group = rng.integers(0, G, size=N).astype(np.int32)
    focal = np.flatnonzero(group == 0)
    cond = np.flatnonzero(group == 1)
    if n_focal is not None:
        focal = focal[:n_focal]
    if n_cond is not None:
        cond = cond[:n_cond]
    return dict(parents=parents, branch_lengths=bls, factors=factors, blocks=blocks, num_blocks=num_blocks,
                group_of_hap=group, num_groups=G, focal=focal, cond=cond, sample_ages=ages)


def default_epochs(years_per_gen=28.0, lineage_bin=4.0):
    """The 31-epoch default grid and the focal epochs as the reference builds them (coal.cpp:5130-5156), in float32."""
    log_10 = np.float32(np.log(10))
    ep = [0.0, 1e3 / years_per_gen]
    for e in range(2, 30):
        ep.append(np.exp(float(log_10) * (3.0 + 4.0 * (e - 1.0) / 28.0)) / years_per_gen)
    ep.append(1e8 / years_per_gen)
    efocal = np.array([0.0, np.exp(np.float32(log_10 * np.float32(lineage_bin)))], dtype=np.float32) / np.float32(years_per_gen)
    return np.array(ep, dtype=np.float32), efocal.astype(np.float32)


def assert_close(a, b, rel=1e-12):
    """Zeros identical, everything else within rel."""
    assert a.shape == b.shape
    za, zb = a == 0.0, b == 0.0
    assert (za == zb).all(), np.argwhere(za != zb)[:5]
    m = ~za
    if m.any():
        r = np.abs(a[m] - b[m]) / np.abs(b[m])
        assert r.max() <= rel, r.max()


def accumulate_in_child(tmpdir, inp, epochs, efocal, device, timeout, env=None):
    """colate_amd.condcoal_accumulate in a child process under a time limit (the GPU steps of the tests): (num, denom).
    env: variables added to the child's environment (COLATE_CONDCOAL_CHUNK_TREES, say)."""
    import sys
    tag = f"{os.getpid()}_{random.getrandbits(32)}"
    src = os.path.join(str(tmpdir), f"in_{tag}.npz")
    dst = os.path.join(str(tmpdir), f"out_{tag}.npz")
    arrays = {k: np.asarray(v) for k, v in inp.items() if v is not None}
    np.savez(src, epochs=epochs, efocal=efocal, **arrays)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), src, dst, "1" if device else "0"], capture_output=True,
                       text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = np.load(dst)
    return out["num"], out["denom"]


if __name__ == "__main__":  # the child of accumulate_in_child
    import sys
    sys.path.insert(0, ROOT)
    import colate_amd

    z = np.load(sys.argv[1])
    kw = {k: z[k] for k in ("parents", "branch_lengths", "factors", "blocks", "group_of_hap", "focal", "cond")}
    num, den = colate_amd.condcoal_accumulate(num_blocks=int(z["num_blocks"]), num_groups=int(z["num_groups"]),
                                              sample_ages=z["sample_ages"] if "sample_ages" in z.files else None,
                                              epochs=z["epochs"], epochs_focal=z["efocal"], device=sys.argv[3] == "1", **kw)
    np.savez(sys.argv[2], num=num, denom=den)
