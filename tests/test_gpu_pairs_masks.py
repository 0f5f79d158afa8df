"""GPU: `Colate --pairs` with per-pair masks and .coal warm starts against the REFERENCE run once per pair (fixture pairs_masks):
iteration counts and .coal tokens per pair, age sampling on the device, and the per-pair starting rates in every EM branch."""
import os
import subprocess

import numpy as np
import pytest

import golden_lib as gl
import pairs_masks_lib as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate")


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    assert colate_amd.device_count() >= 1
    return colate_amd


def _run(args, cwd, **env):
    r = subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stderr


def test_pairs_masks_drop_in(ca, tmp_path):
    """Masks on both samples, on one, on none; masks shared between pairs; coal= for a modern and a 7000-year-old pair and together
    with masks; two launches (--bins 3,7,0.2 and the epochs of prev.coal): every pair's iteration counts are the reference's, and
    so is every .coal token the oracle finds pinned.  The ages are sampled on the device with no pair handed back, and the tables
    equal those of the host's sampling (COLATE_DEVICE_FILL=0)."""
    meta = pm.stage(tmp_path)
    common = ["--mode", "mut", "--mut", "P"] + meta["common_args"]
    B = int(common[common.index("--num_bootstraps") + 1])
    bins = common[common.index("--bins") + 1]
    err = _run(common + ["--pairs", "pairs.txt", "--counts_out", "x"], tmp_path, COLATE_TIMING="1")
    assert "age sampling on the GPU" in err and "0 pair(s) redone" in err, err[-1500:]
    lines = err.split("\n")
    tables = {}
    for k, p in enumerate(meta["pairs"]):
        got = [int(l.rsplit(" ", 1)[1]) for l in lines if l.startswith(f"Pair {k + 1} Bootstrap ")]
        assert got == p["iterations"], (p["output"], got)
        mine = (tmp_path / (p["output"] + ".coal")).read_text().split("\n")
        ref = (tmp_path / f"expected_{p['output']}.coal").read_text().split("\n")
        tables[p["output"]] = (tmp_path / (p["output"] + ".counts")).read_text()
        grid, csh, cns = gl.read_counts(tmp_path / (p["output"] + ".counts"), B)
        ep, ep_null, kw = pm.epochs_of(p, bins, tmp_path)
        note = [l for l in lines if l.startswith(f"Note: pair {k + 1}: the last ")]
        k_cli = int(note[0].split()[5]) if note else 0
        pm.assert_coal_is_the_references(mine, ref, grid, csh, cns, ep, ep_null, pm.age_of(p), k_cli, kw)
    err = _run(common + ["--pairs", "pairs.txt", "--counts_out", "x"], tmp_path, COLATE_TIMING="1", COLATE_DEVICE_FILL="0")
    assert "age sampling on the host (COLATE_DEVICE_FILL=0)" in err, err[-800:]
    for p in meta["pairs"]:
        assert (tmp_path / (p["output"] + ".counts")).read_text() == tables[p["output"]], p["output"]


@pytest.mark.parametrize("how", [["--devices", "1"], ["--ranks", "1"], ["--devices", "2"], ["--ranks", "2"]])
def test_pairs_masks_warm_starts_in_every_em_branch(ca, how, tmp_path):
    """The starting rates go per pair into the rows branch (--devices N: colate_em_batch_rows_sharded) and the ranked branch
    (--ranks N: the all-gather entry point; with one rank a communicator of one, with two the groups of each launch sharded over
    the ranks) as into the default one: the same .coal files.  N = 2 needs two visible GPUs (runs on the multi-GPU node)."""
    if int(how[1]) > 1 and ca.device_count() < int(how[1]):
        pytest.skip(f"needs {how[1]} visible GPUs (runs on the multi-GPU node)")
    meta = pm.stage(tmp_path)
    common = ["--mode", "mut", "--mut", "P"] + meta["common_args"]
    _run(common + ["--pairs", "pairs.txt"], tmp_path)
    want = {p["output"]: (tmp_path / (p["output"] + ".coal")).read_text() for p in meta["pairs"]}
    for p in meta["pairs"]:
        os.remove(tmp_path / (p["output"] + ".coal"))
    _run(common + ["--pairs", "pairs.txt"] + how, tmp_path)
    for p in meta["pairs"]:
        assert (tmp_path / (p["output"] + ".coal")).read_text() == want[p["output"]], p["output"]
