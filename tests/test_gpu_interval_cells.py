"""The interval cells on the device (colate_interval_cells, csrc/interval_cells_kernel.hip) against the host twin in every
bit of kinds, ages, tables and the dropped count, at the sizes at which the kernel takes another path (a wave's batch of 64
records and its edges, chains across lanes and batches, conflicts within a wave, every tile boundary, empty blocks), and
`Colate --mode mut_interval --mut ...` with the cells formed on the device against COLATE_DEVICE_INTERVAL=0."""
import numpy as np
import pytest

import colate_amd
import interval_cells_lib as il
import synth_files

pytestmark = pytest.mark.gpu

CASES = il.cases()


@pytest.fixture(scope="module")
def host():
    """the host twin's results, computed once"""
    return {name: colate_amd.interval_cells(*case, device=False) for name, case in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_twin(name, host):
    got = colate_amd.interval_cells(*CASES[name], device=True)
    il.assert_same_result(got, host[name])
    assert got[0].size > 0


def test_tile_boundary_records_lie_on_both_sides_of_every_boundary():
    """the cells of the tile_boundaries case, from the kernel's tile size: the last two cells of a tile and the first two of the
    next, for every boundary inside the triangle"""
    tile = colate_amd.interval_cells_tile()
    case, cs = il.tile_boundaries(4)
    assert 64 <= tile < il.CELLS
    for t in range(1, (il.CELLS + tile - 1) // tile):
        assert {t * tile - 2, t * tile - 1, t * tile, t * tile + 1} <= set(cs)
    got = colate_amd.interval_cells(*case, device=True)
    assert got[0].size == 2 * len(cs) - int((case[2] == 0).sum()) and got[4] == 0


def test_no_records_on_the_device():
    kinds, a0, a1, tables, dropped = colate_amd.interval_cells([], [], [], [], [], 3, device=True)
    assert kinds.size == 0 and tables.shape == (3, 0) and dropped == 0


def test_cli_cells_on_the_device_equal_the_host_twin(tmp_path):
    synth_files.write_inputs(str(tmp_path), chroms=("1",), snps_per_chr=1500)
    args = ["--mut", "P", "--chr", "chr.txt", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in", "--bins", "3,7,0.2",
            "--num_bootstraps", "6", "--seed", "3", "--max_iter", "60", "--min_iter", "20"]
    dev = il.run_cli(args + ["-o", "dev", "--write_rows", "dev_rows.txt"], tmp_path, device=True)
    assert dev.returncode == 0, dev.stderr[-2000:]
    hst = il.run_cli(args + ["-o", "hst", "--write_rows", "hst_rows.txt"], tmp_path, device=False)
    assert hst.returncode == 0, hst.stderr[-2000:]
    assert (tmp_path / "dev.coal").read_bytes() == (tmp_path / "hst.coal").read_bytes()
    assert (tmp_path / "dev_rows.txt").read_bytes() == (tmp_path / "hst_rows.txt").read_bytes()
    boot = lambda r: [ln for ln in r.stderr.splitlines() if ln.startswith(("Bootstrap ", "Number of ", "SNPs beyond"))]  # noqa: E731
    assert boot(dev) == boot(hst) and len(boot(dev)) == 9
    assert "on the host" not in dev.stderr
    assert "interval cells on the host (COLATE_DEVICE_INTERVAL=0)" in hst.stderr and "interval fit on the host" in hst.stderr
