"""The pair walk on the device (interval_walk_kernel.hip: count pass, write pass, one workgroup per (pair, chromosome))
against its host twin in every byte, on the cases of interval_walk_lib (rows on the edges of the kernel's tile, the carry
across tiles, masks, equal positions, the rounding of the counts, blocks); colate_interval_fit_samples on the device against
colate_interval_fit_groups on the device fed with the host twin's records, in every bit, chunked and not; and
`Colate --mode mut_interval --samples` on the device against `--pairs` on the device and against the host-only run."""
import pytest

import colate_amd
import interval_cells_lib as il
import interval_groups_lib as gl
import interval_walk_lib as wl

SAMPLES, EXPANDED, run_samples = wl.SAMPLES, wl.EXPANDED, wl.run_samples

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(wl.cases()))
def test_device_walk_equals_the_host_twin(name):
    c = wl.cases()[name]
    wl.assert_same_walk(wl.walk(c, device=True), wl.walk(c, device=False))


def test_device_walk_with_exact_room_and_without():
    c = wl.cases()["sizes"]
    host = wl.walk(c, device=False)
    total = int(host[0][-1])
    wl.assert_same_walk(wl.walk(c, device=True, cap=total), host)
    with pytest.raises(colate_amd.ColateError, match=f"needed: {total}"):
        wl.walk(c, device=True, cap=total - 1)


@pytest.mark.parametrize("name", ["sizes", "masks", "blocks", "counts", "carry"])
def test_fit_samples_equals_fit_groups_on_the_host_twins_records(name):
    c = wl.cases()[name]
    dev = wl.fit_samples(c, device=True)
    wl.assert_same_fit(dev, wl.fit_groups_on(wl.walk(c, device=False), device=True))
    wl.assert_same_fit(dev, wl.fit_samples(c, device=False))


@pytest.fixture(scope="module")
def many():
    c = wl.many_records_case()
    host = wl.walk(c, device=False)
    fit = dict(max_iter=12, min_iter=4)
    return c, host, fit, wl.fit_groups_on(host, device=True, **fit)


def test_many_records_device_walk(many):
    c, host, fit, want = many
    assert host[1].tolist() == [1, 1, 1, 3, 1] and (host[0][1:] - host[0][:-1] >= 15000).all()
    wl.assert_same_walk(wl.walk(c, device=True), host)


def chunks(nb, recs, seg_budget, rec_budget):
    """the chunking rule of colate_interval_fit_samples: runs of consecutive pairs within both budgets, a larger pair alone"""
    out, g = [], 0
    while g < len(nb):
        g0, segs, n = g, nb[g], recs[g]
        g += 1
        while g < len(nb) and segs + nb[g] <= seg_budget and n + recs[g] <= rec_budget:
            segs, n = segs + nb[g], n + recs[g]
            g += 1
        out.append(list(range(g0, g)))
    return out


@pytest.mark.parametrize("env", [{"COLATE_INTERVAL_GROUPS_CELLS_MB": "1"}, {"COLATE_INTERVAL_WALK_RECS_MB": "1"}, {}])
def test_three_chunks_change_no_bit(many, monkeypatch, env):
    """a megabyte of dense cell sums holds three segments: {0, 1, 2}, {3}, {4}; a megabyte of records two pairs: {0, 1},
    {2, 3}, {4}; and the default budgets, one chunk"""
    c, host, fit, want = many
    nb, recs = host[1].tolist(), (host[0][1:] - host[0][:-1]).tolist()
    seg = (1 << 20) // (2 * il.CELLS * 8) if "COLATE_INTERVAL_GROUPS_CELLS_MB" in env else 10 ** 9
    rec = (1 << 20) // 28 if "COLATE_INTERVAL_WALK_RECS_MB" in env else 10 ** 12
    assert len(chunks(nb, recs, seg, rec)) == (3 if env else 1)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wl.assert_same_fit(wl.fit_samples(c, device=True, **fit), want)


# ------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("samples_cli_gpu")
    gl.cli_inputs(d)
    return d


def test_cli_samples_on_the_device(cli_dir):
    d = cli_dir
    dev = run_samples(d, SAMPLES, "D", device=True)
    assert dev.returncode == 0, dev.stderr[-2000:]
    assert "4 samples and 1 masks staged, 5 pairs walked on the device" in dev.stderr and "on the host" not in dev.stderr
    host = run_samples(d, SAMPLES, "H", device=False)
    gl.write_list(d / "expanded.txt", EXPANDED, prefix="P_")
    pairs = gl.run_pairs(d, "expanded.txt", device=True)
    fall = run_samples(d, SAMPLES, "F", device=True, env={"COLATE_DEVICE_INTERVAL_WALK": "0"})
    assert host.returncode == 0 and pairs.returncode == 0 and fall.returncode == 0, (host.stderr[-800:], pairs.stderr[-800:], fall.stderr[-800:])
    assert "pairs walked on the host through the engine (COLATE_DEVICE_INTERVAL_WALK=0)" in fall.stderr and "staged" not in fall.stderr
    for i, pair in enumerate(EXPANDED):
        want = (d / f"D_{pair[2]}.coal").read_bytes()
        assert want == (d / f"P_{pair[2]}.coal").read_bytes(), pair[2]
        assert want == (d / f"H_{pair[2]}.coal").read_bytes(), pair[2]
        assert want == (d / f"F_{pair[2]}.coal").read_bytes(), pair[2]
        assert gl.pair_lines(dev.stderr, i + 1, 5) == gl.pair_lines(pairs.stderr, i + 1, 5) == gl.pair_lines(host.stderr, i + 1, 5)
