"""colate_interval_fit_groups on the device -- the cells kernels over (group, block) segments, the row pick
(interval_rows_kernel.hip), the grouped row bootstrap and the grouped fit -- against its host twin (math=1) and against the
existing device calls interval_cells -> bootstrap_em_interval_batch group by group: R, dropped, rates, iteration counts,
log-likelihoods and flags in every bit.  And `Colate --mode mut_interval --pairs` on the device against the same run on the
host twin.  Small shapes throughout: max_iter <= 60."""
import numpy as np
import pytest

import colate_amd
import interval_cells_lib as il
import interval_groups_lib as gl

pytestmark = pytest.mark.gpu


def check(groups, ep, init_rates=None, **fit):
    fit = dict(gl.FIT, **fit)
    dev = colate_amd.interval_fit_groups(groups, ep, init_rates=init_rates, **fit)
    gl.assert_same(dev, colate_amd.interval_fit_groups(groups, ep, init_rates=init_rates, device=False, math=1, **fit))
    gl.assert_same(dev, gl.composed(groups, ep, device=True, init_rates=init_rates, **fit))
    return dev


def five_groups(B):
    """nb = 1, 3, 5, 2, 1; the group in the middle has no records"""
    return [gl.with_weights(il.random_records(60, 1, 41), B, 1), gl.with_weights(il.random_records(40, 3, 42, empty=(1,)), B, 2),
            gl.with_weights(gl.no_records(5), B, 3), gl.with_weights(il.random_records(50, 2, 44), B, 4),
            gl.with_weights(il.random_records(70, 1, 45), B, 5)]


@pytest.mark.parametrize("B", [1, 5])
def test_one_group(B):
    R = check([gl.with_weights(il.random_records(80, 2, 31), B, 5)], gl.epochs23())[0]
    assert R[0] > 8


@pytest.mark.parametrize("B", [1, 5])
def test_five_groups_with_an_empty_one_in_the_middle(B):
    groups = five_groups(B)
    R, dropped, rates, iters, ll, flags = check(groups, gl.epochs23())
    assert [g[5] for g in groups] == [1, 3, 5, 2, 1] and R[2] == 0 and (R[[0, 1, 3, 4]] > 0).all()
    assert (rates[2] == colate_amd.DEFAULT_INIT_RATE).all() and not iters[2].any() and not ll[2].any() and not flags[2].any()


def test_four_groups_of_1_3_5_and_2_blocks():
    check(gl.four_groups(3), gl.epochs23())


def test_the_chunks_change_no_bit(monkeypatch):
    """1 MB holds three segments of dense sums: nb = 1, 3, 5, 2, 1 fall into the chunks {0}, {1}, {2}, {3, 4}"""
    groups, ep = five_groups(5), gl.epochs23()
    whole = colate_amd.interval_fit_groups(groups, ep, **gl.FIT)
    monkeypatch.setenv("COLATE_INTERVAL_GROUPS_CELLS_MB", "1")
    assert 3 * 2 * il.CELLS * 8 <= (1 << 20) < 4 * 2 * il.CELLS * 8
    gl.assert_same(colate_amd.interval_fit_groups(groups, ep, **gl.FIT), whole)
    monkeypatch.setenv("COLATE_INTERVAL_GROUPS_CELLS_MB", "0")  # every group alone
    gl.assert_same(colate_amd.interval_fit_groups(groups, ep, **gl.FIT), whole)


def test_the_scripted_record_sets_side_by_side():
    """rows on both sides of every tile edge of the cells kernel (the ranking runs across the triangular order), the special
    records, a block with only dropped records and an empty block, in one launch"""
    c = il.cases()
    names = ["tile_boundaries", "special", "block_all_dropped", "middle_block_empty"]
    groups = [gl.with_weights(c[n], 2, 50 + i) for i, n in enumerate(names)]
    R, dropped = check(groups, gl.epochs23())[:2]
    assert R[0] == 2 * len(set(il.tile_boundaries(4)[1])) and dropped[1] == 2 and dropped[2] > 0


def test_row_counts_around_the_waves_of_a_group_and_the_rows_in_registers():
    """R of 1, 7, 8, 9 (eight calls at a time) and 511, 512, 513 (64 x 8 rows stay in registers), each group exactly that many"""
    want = [1, 7, 8, 9, 511, 512, 513]
    groups = [gl.with_weights(gl.one_per_cell(R, 60 + R, nb=1 + i % 3), 2, 70 + i) for i, R in enumerate(want)]
    R = check(groups, gl.epochs23(), max_iter=12, min_iter=4)[0]
    assert R.tolist() == want


def test_the_one_wave_layout_at_300_epochs():
    ep = np.concatenate([[0.0], np.geomspace(10.0, 1e7, 299)])
    assert colate_amd.em_interval_batch_waves(ep.size) == 1
    groups = [gl.with_weights(il.random_records(30, 2, 81), 2, 8), gl.with_weights(gl.no_records(1), 2, 9),
              gl.with_weights(gl.one_per_cell(70, 82), 2, 10)]
    R = check(groups, ep, max_iter=12, min_iter=4)[0]
    assert R[1] == 0 and R[2] == 70


# ------------------------------------------------------------------ the command line
def test_cli_pairs_on_the_device_write_the_bytes_of_the_host_twin(tmp_path):
    gl.cli_inputs(tmp_path)
    gl.write_list(tmp_path / "host.txt", gl.SIX_PAIRS, prefix="host_")
    gl.write_list(tmp_path / "dev.txt", gl.SIX_PAIRS, prefix="dev_")
    host = gl.run_pairs(tmp_path, "host.txt", device=False)
    dev = gl.run_pairs(tmp_path, "dev.txt", device=True)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-1500:], dev.stderr[-1500:])
    assert "on the host" in host.stderr and "on the host" not in dev.stderr
    for pair in gl.SIX_PAIRS:
        assert (tmp_path / f"dev_{pair[2]}.coal").read_bytes() == (tmp_path / f"host_{pair[2]}.coal").read_bytes(), pair[2]
    for i in range(len(gl.SIX_PAIRS)):
        assert gl.pair_lines(dev.stderr, i + 1, 6) == gl.pair_lines(host.stderr, i + 1, 6)
