"""The interval cells on the host: the threshold table against a Python restatement of the age bin, the host twin
(colate_interval_cells_host) against an ordered plain loop in every bit, row order and row set, every refused argument, the
anchor to the point path (`Colate --mode mut` accounts for the same total weight per kind on the same inputs), and `Colate
--mode mut_interval --mut ...` on the host twin: --write_rows fed back through --rows gives the same .coal bytes, masks change
the totals as they change `--mode mut`'s, the bad option combinations."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import colate_amd
import golden_lib as gl
import interval_cells_lib as il
import synth_files
from colate_amd._lib import lib

EINVAL = -1


# ------------------------------------------------------------------ thresholds
def test_thresholds_are_the_steps_of_the_age_bin():
    T = il.thresholds()
    assert T.dtype == np.float32 and T.size == il.BINS
    assert (np.diff(T) > 0).all()
    for n in range(1, il.BINS + 1):
        t = T[n - 1]
        assert il.bin_restated(t) == n, n
        assert il.bin_restated(np.nextafter(t, np.float32(0))) == n - 1, n


def test_table_bin_equals_restatement_on_random_floats():
    rng = np.random.default_rng(1)
    x = np.concatenate([[0.0], np.exp(rng.uniform(math.log(1e-3), math.log(1e7), 100000))]).astype(np.float32)
    table = np.searchsorted(il.thresholds(), x, side="right")
    want = np.array([il.bin_restated(v) for v in x])
    assert np.array_equal(table, want)
    assert want.min() == 0 and want.max() > 180  # (the sample covers the grid)


# ------------------------------------------------------------------ the twin against the ordered loop
CASES = il.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_ordered_loop(name):
    case = CASES[name]
    got = colate_amd.interval_cells(*case, device=False)
    il.assert_same_result(got, il.loop_cells(*case))
    assert got[3].shape == (case[5], got[0].size)


def test_the_order_of_addition_matters_for_the_chosen_weights():
    """the loop in reversed record order differs in at least one cell: a wrong order in the twin or the kernel would show"""
    for name in ("one_cell_130", "random_5x2000", "alternating"):
        case = CASES[name]
        fwd = il.loop_cells(*case)
        rev = il.loop_cells(*case, order=range(len(case[0]) - 1, -1, -1))
        assert il.same_bits(fwd[0], rev[0]) and fwd[3].shape == rev[3].shape
        assert not il.same_bits(fwd[3], rev[3]), name
        assert np.allclose(fwd[3], rev[3], rtol=1e-12, atol=0)


def test_special_records():
    kinds, a0, a1, tables, dropped = colate_amd.interval_cells(*il.special_records(), device=False)
    g = il.grid()
    assert dropped == 2
    # (0, 0) from the record with both ages 0, the F-path row from 0 and the point row, of both kinds
    want = [(0.0, 0.0), (0.0, g[il.bin_restated(np.float32(800.0))]), (g[il.bin_restated(np.float32(500.0))],) * 2]
    assert list(zip(a0, a1)) == want + want and kinds.tolist() == [0] * 3 + [1] * 3
    assert tables.tolist() == [[0.25, 1.5, 2.0, 4.0, 0.5, 0.125]]


def test_block_with_only_dropped_records_and_empty_block():
    case = CASES["block_all_dropped"]
    kinds, a0, a1, tables, dropped = colate_amd.interval_cells(*case, device=False)
    assert (tables[1] == 0).all() and (tables[2] == 0).all() and tables[0].sum() > 0
    assert dropped >= 100


def test_row_order_and_row_set():
    """kind, then bb, then be; a cell positive in one block only appears; a cell of zero weights does not"""
    T = il.thresholds()
    a = [il.age_in_bin(b) for b in (0, 5, 5, 90, 90, 17)]
    e = [il.age_in_bin(b) for b in (184, 9, 7, 90, 100, 30)]
    begin, end = np.array(a * 2, dtype=np.float32), np.array(e * 2, dtype=np.float32)
    w_sh = np.array([1, 2, 3, 4, 5, 0] + [0] * 6, dtype=float)  # (shared: positive in block 0 only; the cell (17, 30) never)
    w_ns = np.array([0] * 6 + [1, 2, 3, 4, 5, 6], dtype=float)  # (not shared: in block 2 only)
    block = np.array([0] * 6 + [2] * 6, dtype=np.int32)
    kinds, a0, a1, tables, dropped = colate_amd.interval_cells(begin, end, w_sh, w_ns, block, 3, device=False)
    g = il.grid()
    cells = [(0, 184), (5, 7), (5, 9), (90, 90), (90, 100)]
    assert kinds.tolist() == [0] * 5 + [1] * 6
    assert list(zip(a0, a1)) == [(g[b], g[c]) for b, c in cells] + [(g[b], g[c]) for b, c in cells[:1] + [(5, 7), (5, 9), (17, 30)] + cells[3:]]
    assert tables[0].tolist() == [1, 3, 2, 4, 5] + [0] * 6 and (tables[1] == 0).all()
    assert tables[2].tolist() == [0] * 5 + [1, 3, 2, 6, 4, 5] and dropped == 0
    assert T[183] <= end[0]


def test_no_records_and_room():
    kinds, a0, a1, tables, dropped = colate_amd.interval_cells([], [], [], [], [], 2, device=False)
    assert kinds.size == 0 and tables.shape == (2, 0) and dropped == 0
    case = CASES["nb1"]
    R = colate_amd.interval_cells(*case, device=False)[0].size
    il.assert_same_result(colate_amd.interval_cells(*case, device=False, max_rows=R), colate_amd.interval_cells(*case, device=False))
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.interval_cells(*case, device=False, max_rows=R - 1)
    assert e.value.code == EINVAL


# ------------------------------------------------------------------ refusals
def _bad_calls():
    begin, end, w_sh, w_ns, block, nb = il.random_records(20, 3, 9)

    def with_(**kw):
        d = dict(begin=begin.copy(), end=end.copy(), w_sh=w_sh.copy(), w_ns=w_ns.copy(), block=block.copy(), nb=nb)
        for k, (i, v) in kw.items():
            if k == "nb":
                d["nb"] = v
            else:
                d[k][i] = v
        return d

    return {
        "nan begin": with_(begin=(4, np.nan)),
        "nan end": with_(end=(4, np.nan)),
        "negative begin": with_(begin=(0, -1.0)),
        "negative end": with_(begin=(7, 0.0), end=(7, -2.0)),
        "begin > end": with_(begin=(3, 5000.0), end=(3, 50.0)),
        "negative shared weight": with_(w_sh=(2, -1e-9)),
        "infinite shared weight": with_(w_sh=(2, np.inf)),
        "nan not-shared weight": with_(w_ns=(59, np.nan)),
        "negative not-shared weight": with_(w_ns=(0, -3.0)),
        "blocks out of order": with_(block=(25, 0)),
        "block beyond nb": with_(block=(59, 3)),
        "negative block": with_(block=(0, -1)),
        "nb 0": with_(nb=(0, 0)),
        "nb below the blocks": with_(nb=(0, 2)),
    }


BAD = _bad_calls()


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(BAD))
def test_refused_arguments_leave_the_outputs_alone(name, host):
    """COLATE_EINVAL before anything is staged: the device call refuses the same arguments without asking for a device"""
    d = BAD[name]
    recs = np.zeros(d["begin"].size, dtype=colate_amd.api.INTERVAL_REC)
    recs["begin"], recs["end"], recs["w_sh"], recs["w_ns"] = d["begin"], d["end"], d["w_sh"], d["w_ns"]
    block = np.ascontiguousarray(d["block"], dtype=np.int32)
    cap = 2 * recs.size
    kinds = np.full(cap, -7, dtype=np.int32)
    a0, a1, tables = np.full(cap, -7.0), np.full(cap, -7.0), np.full(3 * cap, -7.0)
    dropped = ctypes.c_longlong(-7)
    fn = lib.colate_interval_cells_host if host else lib.colate_interval_cells
    rc = fn(recs.size, recs.ctypes.data, block.ctypes.data, d["nb"], cap, kinds.ctypes.data, a0.ctypes.data, a1.ctypes.data,
            tables.ctypes.data, ctypes.addressof(dropped))
    assert rc == EINVAL, (name, rc)
    assert (kinds == -7).all() and (a0 == -7).all() and (a1 == -7).all() and (tables == -7).all() and dropped.value == -7


# ------------------------------------------------------------------ the command line on the host twin
FIT = ["--bins", "3,7,0.2", "--num_bootstraps", "6", "--seed", "3", "--max_iter", "60", "--min_iter", "20"]
INPUTS = ["--mut", "P", "--chr", "chr.txt", "--target_tmp", "T.colate.in", "--reference_tmp", "R.colate.in"]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """tests/synth_files inputs, two chromosomes of the default size (rows with age_begin = 0 among them, no age beyond the
    grid), and the host-twin run with --write_rows that several tests read"""
    d = tmp_path_factory.mktemp("interval_cells")
    synth_files.write_inputs(str(d))
    r = il.run_cli(INPUTS + FIT + ["-o", "mi", "--write_rows", "rows.txt"], d, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    return d, r


def test_cli_stderr_lines(synth):
    d, r = synth
    lines = r.stderr.splitlines()
    i = [k for k, ln in enumerate(lines) if ln.startswith("Number of blocks: ")][0]
    assert lines[i + 1].startswith("Number of rows: ") and lines[i + 2] == "SNPs beyond the age grid: 0"
    assert lines[i - 1] == "interval cells on the host (COLATE_DEVICE_INTERVAL=0)"
    assert lines[i + 3].startswith("Maximising likelihood using EM")
    assert sum(ln.startswith("Bootstrap ") for ln in lines) == 6
    total, n_rows, blocks = il.read_rows_file(d / "rows.txt")
    assert n_rows == il.stderr_count(r, "Number of rows") and blocks == list(range(il.stderr_count(r, "Number of blocks")))


def test_cli_rows_file_round_trip_gives_the_same_coal(synth):
    d, _ = synth
    r = il.run_cli(["--rows", "rows.txt"] + FIT + ["-o", "back"], d, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (d / "back.coal").read_bytes() == (d / "mi.coal").read_bytes()
    rates = np.array([[float(x) for x in ln.split()[2:]] for ln in (d / "mi.coal").read_text().splitlines()[2:]])
    assert rates.shape[0] == 6 and np.isfinite(rates).all() and (rates >= 0).all() and (rates > 0).any()


def _mut_totals(d, extra=()):
    """per kind what `--mode mut` accounts for on the same inputs: with one bootstrap every block weighs 1, the count tables are
    the sums of the per-block tables, the shared one with the redistributed emp row (--counts_out: 17 significant digits)"""
    args = ["--mode", "mut"] + INPUTS + list(extra) + ["--bins", "3,7,0.2", "--num_bootstraps", "1", "--seed", "3", "-o", "pt",
                                                       "--counts_out", "pt.counts", "--counts_only"]
    r = subprocess.run([il.CLI] + args, cwd=str(d), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _, csh, cns = gl.read_counts(d / "pt.counts", 1)
    return csh.sum(), cns.sum(), il.stderr_count(r, "Number of blocks")


def test_anchor_total_weight_per_kind_equals_the_point_path(synth):
    """Both sides sum the same SNP weights, at most a few 1e5 non-negative doubles in different orders (the point path in
    hundredths per SNP, and its emp row through a normalised redistribution): they differ by about n * 2^-53 ~ 1e-11
    relative at the most; the bound is 1e-9.  Both sides are read from text with 17 significant digits, which is exact."""
    d, r = synth
    sh, ns, nb = _mut_totals(d)
    total, _, blocks = il.read_rows_file(d / "rows.txt")
    print("shared", total["shared"], sh, "notshared", total["notshared"], ns)
    assert nb == len(blocks) == il.stderr_count(r, "Number of blocks")
    assert sh > 100 and ns > 100
    assert abs(total["shared"] - sh) <= 1e-9 * sh
    assert abs(total["notshared"] - ns) <= 1e-9 * ns


def test_cli_masks_change_the_totals_as_they_change_mode_mut(synth, tmp_path):
    d, r0 = synth
    for c in ("1", "2"):
        il.write_mask(d / f"M_chr{c}.fa", 20_000_000 if c == "1" else 8_000_000)
        il.write_mask(d / f"N_chr{c}.fa", 3_000_000)
    masks = ["--target_mask", "M", "--reference_mask", "N"]
    r = il.run_cli(INPUTS + masks + FIT + ["-o", "masked", "--write_rows", "rows_masked.txt"], d, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    sh, ns, nb = _mut_totals(d, masks)
    total, n_rows, blocks = il.read_rows_file(d / "rows_masked.txt")
    total0, n_rows0, _ = il.read_rows_file(d / "rows.txt")
    assert il.stderr_count(r, "Number of blocks") == nb == len(blocks) == il.stderr_count(r0, "Number of blocks")
    assert il.stderr_count(r, "Number of rows") == n_rows < n_rows0 == il.stderr_count(r0, "Number of rows")
    assert il.stderr_count(r, "SNPs beyond the age grid") == 0
    assert abs(total["shared"] - sh) <= 1e-9 * sh and abs(total["notshared"] - ns) <= 1e-9 * ns
    assert total["shared"] < 0.95 * total0["shared"] and total["notshared"] < 0.95 * total0["notshared"]


def test_cli_counts_snps_beyond_the_grid_and_keeps_empty_blocks(tmp_path):
    """5 used-looking SNPs pushed beyond the grid are dropped and counted; a chromosome whose SNPs are all masked leaves
    a block without a positive cell, which --write_rows keeps (a line of weight 0), so that --rows gives the same .coal"""
    synth_files.write_inputs(str(tmp_path), snps_per_chr=400, span=40_000_000)
    r = il.run_cli(INPUTS + FIT + ["-o", "a"], tmp_path, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    synth_files.push_beyond_the_age_grid(str(tmp_path / "P_chr1.mut"), 5)
    il.write_mask(tmp_path / "M_chr1.fa", 1000)
    il.write_mask(tmp_path / "M_chr2.fa", 41_000_000)
    args = INPUTS + ["--target_mask", "M"] + FIT
    r2 = il.run_cli(args + ["-o", "b", "--write_rows", "rows.txt"], tmp_path, device=False)
    assert r2.returncode == 0, r2.stderr[-2000:]
    dropped = il.stderr_count(r2, "SNPs beyond the age grid")
    assert 1 <= dropped <= 5 and il.stderr_count(r, "SNPs beyond the age grid") == 0
    nb = il.stderr_count(r2, "Number of blocks")
    zero = [ln.split() for ln in open(tmp_path / "rows.txt") if ln.split()[-1] == "0"]
    assert len(zero) >= 1 and il.read_rows_file(tmp_path / "rows.txt")[2] == list(range(nb))
    r3 = il.run_cli(["--rows", "rows.txt"] + FIT + ["-o", "c"], tmp_path, device=False)
    assert r3.returncode == 0, r3.stderr[-2000:]
    assert (tmp_path / "c.coal").read_bytes() == (tmp_path / "b.coal").read_bytes()


@pytest.mark.parametrize("args,msg", [
    (["--rows", "rows.txt", "--mut", "P"], "--rows cannot be combined with --mut, --target_tmp or --reference_tmp"),
    (["--rows", "rows.txt", "--target_tmp", "T.colate.in"], "--rows cannot be combined"),
    (["--rows", "rows.txt", "--reference_tmp", "R.colate.in"], "--rows cannot be combined"),
    (INPUTS + ["--target_age", "7000"], "--target_age and --reference_age are not supported"),
    (INPUTS + ["--reference_age", "100"], "--target_age and --reference_age are not supported"),
    (["--mut", "P", "--target_tmp", "T.colate.in"], "needs --rows FILE (or --mut, --target_tmp and --reference_tmp)"),
])
def test_cli_bad_option_combinations(synth, args, msg):
    d, _ = synth
    r = il.run_cli(args + FIT + ["-o", "bad"], d, device=False)
    assert r.returncode == 1 and msg in r.stderr, r.stderr[-800:]
    assert not (d / "bad.coal").exists()
