"""The pairs_masks fixture (tests/golden/make_golden_pairs_masks.py: the reference run once per pair with per-pair masks and .coal
warm starts): staging, the pairs list in the `key=value` grammar, and the comparison of a pair's .coal with the reference's."""
import gzip
import json
import os
import shutil

import numpy as np

import oracle_lib as ol

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs_masks")


def line_of(p):
    """The pairs-list line of fixture pair `p`: names, the ages where the reference run was given them, the keys."""
    toks = [p["target"], p["reference"], p["output"]]
    if p["target_age"] is not None:
        toks += [p["target_age"], p["reference_age"]]
    toks += [f"{k}={v}" for k, v in p["keys"].items()]
    return " ".join(toks) + "\n"


def stage(dst, pairs_file="pairs.txt"):
    """Copies the fixture into `dst` (the .colate.in files decompressed: the reference freads them raw), writes the pairs list and
    returns the case description."""
    os.makedirs(dst, exist_ok=True)
    for f in os.listdir(HERE):
        if f.endswith(".colate.in.gz"):
            with gzip.open(os.path.join(HERE, f), "rb") as g, open(os.path.join(dst, f[:-3]), "wb") as o:
                o.write(g.read())
        else:
            shutil.copy(os.path.join(HERE, f), os.path.join(dst, f))
    meta = json.load(open(os.path.join(HERE, "case.json")))
    with open(os.path.join(dst, pairs_file), "w") as f:
        for p in meta["pairs"]:
            f.write(line_of(p))
    return meta


def age_of(p, years_per_gen=28.0):
    ta = p["target_age"] or "0"
    ra = p["reference_age"] or "0"
    return max(float(np.float32(ta)), float(np.float32(ra))) / years_per_gen


def epochs_of(p, bins, cwd):
    """(epochs, ep_null, EM keyword arguments) of fixture pair `p`: from its coal= file (starting rates too, ep_null = 0) or --bins."""
    age = age_of(p)
    if "coal" in p["keys"]:
        ep, init = ol.epochs_from_coal(os.path.join(str(cwd), p["keys"]["coal"]), age)
        return ep, 0, {"init": init}
    ep, ep_null = ol.epochs_from_bins(bins, age, 28.0)
    return ep, ep_null, {}


def assert_coal_is_the_references(mine, ref, grid, csh, cns, ep, ep_null, age, k_cli, kw={}, min_stable=0.8):
    """`mine` / `ref`: the lines of our .coal and of the reference's for the same inputs; `k_cli` = the number of trailing epochs the
    CLI's note declares unresolved.  Every token the oracle's stable mask (oracle_lib.stable_mask) finds pinned by the reference's
    source must be the reference's; the CLI's note must cover at least the epochs the checker finds unstable."""
    assert mine[:2] == ref[:2] and len(mine) == len(ref)
    B = csh.shape[0]
    r0, _, _, _ = ol.em_batch(grid, csh, cns, ep, **kw)
    mask = ol.stable_mask(grid, csh, cns, ep, r0, **kw)
    first = ep_null if age > 0 else 0  # ancient samples print epochs from ep_null on (coal.cpp:3837)
    unstable = ep.size - mask.sum(axis=1)
    assert mask.mean() > min_stable, mask.mean()
    assert unstable.max() - 1 <= k_cli <= unstable.max() + 3, (k_cli, unstable)
    for b in range(B):
        m_tok, r_tok = mine[2 + b].split(), ref[2 + b].split()
        assert m_tok[:2] == r_tok[:2] and len(m_tok) == len(r_tok)
        for j, e in enumerate(range(first, ep.size)):
            if m_tok[2 + j] != r_tok[2 + j]:
                assert not mask[b, e] and e >= ep.size - k_cli, (b, e, m_tok[2 + j], r_tok[2 + j])
