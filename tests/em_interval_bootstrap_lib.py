"""What the tests of the block bootstrap in front of the interval-dated fit (colate_bootstrap_em_interval_batch, `Colate
--mode mut_interval`) share: small random per-block tables, a rows file with every feature of the format, the CLI runner
and the Python composition that the CLI's output is compared with."""
import os
import subprocess

import numpy as np

import colate_amd
import em_interval_fit_lib as fl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")


def random_tables(E, R, B, nb, seed):
    """rows and grid of em_interval_fit_lib.random_problem; tables[nb][R] with small counts, a quarter of them fractional,
    zeros among them; block weights [B][nb] multinomial as the bootstrap draws them (zeros among them for nb > 1)"""
    k, a0, a1, _, ep, init = fl.random_problem(E, R, 1, seed)
    rng = np.random.default_rng(seed + 1)
    t = rng.integers(0, 4, (nb, R)).astype(float)
    t += (rng.random((nb, R)) < 0.25) * rng.random((nb, R))
    t[0, 0] = max(t[0, 0], 1.0)
    bw = np.stack([np.bincount(rng.integers(0, nb, nb), minlength=nb) for _ in range(B)]).astype(float)
    return k, a0, a1, bw, t, ep, init


def loop_rows(bw, t):
    """W[b][r] = sum_k bw[b][k] * t[k][r] the plain way: from 0.0, k ascending, the product rounded and then added"""
    B, nb = bw.shape
    R = t.shape[1]
    W = np.zeros((B, R))
    for b in range(B):
        for r in range(R):
            acc = np.float64(0.0)
            for k in range(nb):
                acc = acc + np.float64(bw[b, k]) * np.float64(t[k, r])
            W[b, r] = acc
    return W


# (block, kind, age_begin, age_end, weight) in file order: three blocks with non-contiguous ids, not sorted; the cell (40,
# shared 100..2500.5) three times, once spelt differently; both kinds; a point row; an interval into the last epoch of
# --bins 3,7,0.2 (which starts at 1e8 / 28 generations); a weight of zero
ROWS = [
    (40, "shared", "100", "2500.5", "2"),
    (7, "notshared", "30", "30", "1.5"),
    (40, "notshared", "30", "30", "4"),
    (1000, "shared", "5e3", "1e7", "1"),
    (7, "shared", "100", "2500.5", "3"),
    (40, "shared", "1e2", "2500.50", "0.25"),
    (1000, "notshared", "12.5", "700", "2"),
    (7, "notshared", "12.5", "700", "0"),
    (1000, "shared", "800", "800", "6"),
    (40, "shared", "100", "2500.5", "0.125"),
    (7, "shared", "20000", "3.1e5", "2"),
    (40, "notshared", "4000", "90000", "3"),
]


def rows_text(rows=ROWS):
    lines = ["# block kind age_begin age_end weight"]
    for i, r in enumerate(rows):
        if i == 3:
            lines.append("")
        lines.append(" ".join(str(x) for x in r) if i % 2 else "\t".join(str(x) for x in r))
    return "\n".join(lines) + "\n"


def tables_of(rows=ROWS):
    """the format's rule in Python: blocks ascending, triples in order of first appearance, cells summed in file order"""
    blocks = sorted({r[0] for r in rows})
    triples = []
    for _, kind, a0, a1, _ in rows:
        key = (0 if kind == "shared" else 1, float(a0), float(a1))
        if key not in triples:
            triples.append(key)
    t = np.zeros((len(blocks), len(triples)))
    for b, kind, a0, a1, w in rows:
        t[blocks.index(b), triples.index((0 if kind == "shared" else 1, float(a0), float(a1)))] += float(w)
    k = np.array([x[0] for x in triples], dtype=np.int32)
    return k, np.array([x[1] for x in triples]), np.array([x[2] for x in triples]), t


def run_cli(args, cwd, device, timeout=120):
    env = dict(os.environ)
    env.pop("COLATE_DEVICE_INTERVAL", None)
    if not device:
        env["COLATE_DEVICE_INTERVAL"] = "0"
    return subprocess.run([CLI, "--mode", "mut_interval"] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True,
                          env=env, timeout=timeout)


def composed_coal(path, k, a0, a1, t, epochs, init, ep_null, B, seed, **fit):
    """Rng(seed) -> bootstrap_weights -> bootstrap_rows -> em_interval_batch on the host (math=1) -> write_coal"""
    bw = colate_amd.bootstrap_weights(colate_amd.Rng(seed), B, t.shape[0])
    W = colate_amd.bootstrap_rows(bw, t)
    rates, iters, ll, flags = colate_amd.em_interval_batch(k, a0, a1, W, epochs, init, device=False, math=1, **fit)
    colate_amd.write_coal(path, epochs, rates, False, ep_null)
    return rates, iters
