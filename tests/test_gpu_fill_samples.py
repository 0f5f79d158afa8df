"""colate_fill_samples on the GPU against its host twin, bit for bit, and `Colate --mode mut --samples` on the device path
against `--pairs` and the reference's files.  The cases, their edges and the twin's side are in fill_samples_lib.py and
tests/test_fill_samples_cpu.py (which checks that no case but hand_back can pass here through the hand-back)."""
import os

import pytest

import colate_amd
import fill_samples_lib as fl
import golden_lib as gl
import interval_walk_lib as wl
import oracle_lib as ol
import pairs_masks_lib as pm

pytestmark = pytest.mark.gpu

NAMES = sorted(fl.cases())


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_twin_in_every_bit(name):
    """tables, nb, used and the generator's position; handed_back is the twin's near_band.  The walk's edges (W - 1, W, W + 1
    and 3W + 5 rows, carry, masks, equal positions, counts, empty blocks, one row, one base per block), the row-0 kernel's
    (63, 64, 65 and 129 F records in a block, a batch in one bin and one in 64 bins, age_begin 0.0, -0.0 and negative, an
    F record ending beyond the grid, a block without F records), the jobs kernel's (a pair without a used row, a pair of 520
    one-row blocks) and a pair that is handed back beside a clean one are the cases' names."""
    want = fl.twin(name)
    got = fl.fill(fl.cases()[name], device=True)
    fl.assert_same_fill(got, want)
    assert got["handed_back"].tolist() == want["near_band"].tolist() == fl.HANDED_BACK.get(name, [0] * len(want["nb"]))


def test_jobs_case_is_what_it_says():
    got = fl.fill(fl.cases()["jobs"], device=True)
    assert got["nb"].tolist() == [520, 1, 520] and got["used"].tolist() == [520, 0, 520] and (got["handed_back"] == 0).all()
    assert (got["tables"][1] == 0).all()


def test_chunking_changes_no_bit():
    c = wl.many_records_case()
    want = fl.fill(c, device=False)
    assert (want["near_band"] == 0).all()
    counts = {}
    for mb in (None, 1):
        old = os.environ.pop("COLATE_FILL_SAMPLES_RECS_MB", None)
        try:
            if mb:
                os.environ["COLATE_FILL_SAMPLES_RECS_MB"] = str(mb)
            got = fl.fill(c, device=True)
        finally:
            os.environ.pop("COLATE_FILL_SAMPLES_RECS_MB", None)
            if old is not None:
                os.environ["COLATE_FILL_SAMPLES_RECS_MB"] = old
        counts[mb] = colate_amd.fill_samples_chunks()
        fl.assert_same_fill(got, want)
        assert (got["handed_back"] == 0).all()
    assert counts[None] == 1 and counts[1] == fl.chunks_by_rule(want["used"], 1) >= 3, counts


@pytest.mark.parametrize("fixture", sorted(fl.FIXTURES))
def test_samples_cli_writes_the_files_of_pairs_and_of_the_reference(fixture, tmp_path):
    stage, lists = fl.FIXTURES[fixture]
    meta = stage(str(tmp_path))
    common = meta["common_args"]
    B = int(common[common.index("--num_bootstraps") + 1])
    by_output = {p["output"]: p for p in meta["pairs"]}
    # every process of the test side by side: per list `--samples` and `--pairs`, and on the last list the two switches
    names_of = [fl.write_lists(tmp_path, samples, k) for k, (samples, _) in enumerate(lists)]
    runs = [r for k in range(len(lists)) for r in fl.both_runs(common, k, ["--counts_out", "x"])]
    last = len(lists) - 1
    switches = [({"COLATE_DEVICE_FILL_WALK": "0"}, "COLATE_DEVICE_FILL_WALK=0"), ({"COLATE_DEVICE_FILL": "0"}, "COLATE_DEVICE_FILL=0")]
    runs += [(common + ["--samples", f"samples{last}.txt", "-o", f"f{j}"], env) for j, (env, _) in enumerate(switches)]
    done = fl.run_many(tmp_path, runs)
    for k, (samples, in_fixture) in enumerate(lists):
        rs, rp, names = done[2 * k], done[2 * k + 1], names_of[k]
        fl.assert_all_indexed(rp, len(names))
        assert rs.returncode == 0, rs.stderr[-800:]
        n_masks = len({s[2] for s in samples if s[2]})
        assert f"{len(samples)} samples and {n_masks} masks staged, {len(names)} pairs walked and filled on the device (0 handed back to the host)" \
            in rs.stderr, rs.stderr[-800:]
        err = rs.stderr.split("\n")
        for i, name in enumerate(names):
            assert any(l.startswith(f"Pair {i + 1} / {len(names)}: ") for l in err)
            for ext in (".coal", ".counts"):
                mine, theirs = (tmp_path / f"s{k}_{name}{ext}").read_bytes(), (tmp_path / f"e{k}_{name}{ext}").read_bytes()
                assert len(mine) > 100 and mine == theirs, (name, ext)
            if name not in in_fixture:
                continue
            p = by_output[in_fixture[name]]  # ... and the reference's own run of the pair, as test_l3_pairs_drop_in compares
            got = [int(l.rsplit(" ", 1)[1]) for l in err if l.startswith(f"Pair {i + 1} Bootstrap ")]
            assert got == p["iterations"], (name, got)
            mine = (tmp_path / f"s{k}_{name}.coal").read_text().split("\n")
            ref = (tmp_path / f"expected_{p['output']}.coal").read_text().split("\n")
            grid, csh, cns = gl.read_counts(tmp_path / f"s{k}_{name}.counts", B)
            age = pm.age_of(p)
            ep, ep_null = ol.epochs_from_bins(common[common.index("--bins") + 1], age, 28.0)
            note = [l for l in err if l.startswith(f"Note: pair {i + 1}: the last ")]
            pm.assert_coal_is_the_references(mine, ref, grid, csh, cns, ep, ep_null, age, int(note[0].split()[5]) if note else 0)
    for j, (_, why) in enumerate(switches):  # one line each, the same bytes
        r = done[2 * len(lists) + j]
        assert r.returncode == 0, r.stderr[-800:]
        assert f"pairs walked and filled through the engine of --pairs ({why})" in r.stderr and "filled on the device" not in r.stderr
        for name in names_of[last]:
            assert (tmp_path / f"f{j}_{name}.coal").read_bytes() == (tmp_path / f"s{last}_{name}.coal").read_bytes(), (name, why)
