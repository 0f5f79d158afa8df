"""The block bootstrap in front of the interval-dated EM fit on the CPU: colate_bootstrap_rows_host (the host twin of
bootstrap_rows_kernel) against a plain loop in the contract's order, colate_bootstrap_em_interval_batch_host against
colate_em_interval_batch_host on those sums, the refusals, and `Colate --mode mut_interval` on the host twin
(COLATE_DEVICE_INTERVAL=0) against the same steps composed in Python."""
import gzip

import numpy as np
import pytest

import colate_amd
import em_interval_bootstrap_lib as bl
import em_interval_fit_lib as fl

lib = colate_amd.api.lib


@pytest.mark.parametrize("nb", (1, 2, 7))
@pytest.mark.parametrize("R", (1, 9, 130))
def test_bootstrap_rows_equals_a_plain_loop_in_every_bit(nb, R):
    rng = np.random.default_rng(1000 * nb + R)
    t = rng.random((nb, R)) * np.exp(rng.uniform(-20, 20, (nb, R)))  # (products and sums that round)
    bw = rng.integers(0, 4, (3, nb)).astype(float) + (rng.random((3, nb)) < 0.3) * rng.random((3, nb))
    bw[0, nb // 2] = 0.0            # a zero weight
    bw[1] = 0.0                     # a replicate of zeros
    t[:, R // 2] = 0.0              # a zero column
    W = colate_amd.bootstrap_rows(bw, t)
    assert W.shape == (3, R) and fl.same_bits(W, bl.loop_rows(bw, t))
    assert (W[1] == 0.0).all() and (W[:, R // 2] == 0.0).all() and not np.signbit(W).any()


@pytest.mark.parametrize("math", (0, 1))
def test_bootstrap_fit_equals_the_fit_on_those_sums_bit_for_bit(math):
    for E, R, B, nb, seed in ((23, 9, 4, 7, 1), (8, 1, 2, 2, 2), (40, 20, 3, 1, 3)):
        k, a0, a1, bw, t, ep, init = bl.random_tables(E, R, B, nb, seed)
        W = colate_amd.bootstrap_rows(bw, t)
        want = colate_amd.em_interval_batch(k, a0, a1, W, ep, init, 40, 5, 1e-5, device=False, math=math)
        got = colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, init, 40, 5, 1e-5, device=False, math=math)
        fl.assert_same_fit(got, want, (E, R, B, nb))
        assert np.isfinite(got[0]).all() and got[1].min() >= 1


@pytest.mark.parametrize("math", (0, 1))
def test_one_block_with_weight_one_is_the_fit_on_its_table(math):
    k, a0, a1, _, t, ep, init = bl.random_tables(23, 9, 1, 1, 5)
    want = colate_amd.em_interval_batch(k, a0, a1, t[0], ep, init, 30, 5, 1e-5, device=False, math=math)
    got = colate_amd.bootstrap_em_interval_batch(k, a0, a1, [1.0], t, ep, init, 30, 5, 1e-5, device=False, math=math)
    fl.assert_same_fit(got, want)
    assert fl.same_bits(colate_amd.bootstrap_rows([[1.0]], t), t)


def test_refusals_leave_the_outputs_alone():
    k, a0, a1, bw, t, ep, init = bl.random_tables(8, 5, 2, 3, seed=1)
    good = dict(B=2, nb=3, R=5, E=8, kinds=k, a0=a0, a1=a1, bw=bw, t=t, ep=ep, init=init, max_iter=10, min_iter=0, rel_tol=1e-6,
                floor=5e-9)

    def refused(**change):
        a = dict(good, **change)
        for host in (True, False):  # (the checks come before a device is asked for)
            rates, iters = np.full((2, 8), -7.0), np.full(2, -7, dtype=np.int32)
            ll, flags = np.full(2, -7.0), np.full(2, -7, dtype=np.int32)
            arr = [np.ascontiguousarray(a[n], dtype=ty) for n, ty in (("kinds", np.int32), ("a0", float), ("a1", float), ("bw", float),
                                                                      ("t", float), ("ep", float), ("init", float))]
            args = [a["B"], a["nb"], a["R"], a["E"]] + [x.ctypes.data for x in arr] + [
                a["max_iter"], a["min_iter"], a["rel_tol"], a["floor"], rates.ctypes.data, iters.ctypes.data, ll.ctypes.data,
                flags.ctypes.data]
            rc = lib.colate_bootstrap_em_interval_batch_host(*args, 1) if host else lib.colate_bootstrap_em_interval_batch(*args)
            assert rc == -1, (change.keys(), host, rc)
            assert lib.colate_last_error()
            assert (rates == -7.0).all() and (iters == -7).all() and (ll == -7.0).all() and (flags == -7).all()

    def with_value(x, idx, v):
        y = np.array(x, dtype=float)
        y[idx] = v
        return y

    # what the new call adds
    refused(nb=0)
    refused(nb=-1)
    refused(bw=with_value(bw, (1, 2), -1.0))
    refused(bw=with_value(bw, (0, 0), np.inf))
    refused(bw=with_value(bw, (0, 1), np.nan))
    refused(t=with_value(t, (2, 4), -0.5))
    refused(t=with_value(t, (0, 0), np.inf))
    refused(t=with_value(t, (1, 3), np.nan))
    big = with_value(with_value(t, (0, 2), 1.5e308), (1, 2), 1.5e308)
    refused(t=big, bw=np.ones((2, 3)))                   # a sum that overflows
    refused(t=with_value(t, (0, 2), 1e308), bw=with_value(bw, (0, 0), 2.0))  # a product that overflows
    # everything colate_em_interval_batch refuses
    refused(B=0)
    refused(R=0)
    refused(min_iter=-1)
    refused(max_iter=0)
    refused(rel_tol=0.0)
    refused(rel_tol=-1e-7)
    refused(rel_tol=np.inf)
    refused(rel_tol=np.nan)
    refused(floor=-1e-9)
    refused(init=with_value(init, 3, -1e-5))
    refused(init=with_value(init, 0, np.inf))
    refused(init=with_value(init, 7, np.nan))
    refused(a0=with_value(a0, 1, a1[1] * 2))
    refused(a0=with_value(a0, 0, -1.0))
    refused(a1=with_value(a1, 2, np.inf))
    refused(kinds=np.array([0, 1, 2, 0, 1]))
    refused(ep=with_value(ep, 3, ep[1]))                 # epochs that decrease
    # values next to the refused ones pass: the largest finite sums do not overflow
    ok = colate_amd.bootstrap_rows(np.ones((1, 2)), [[8e307], [8e307]])
    assert np.isfinite(ok).all() and ok[0, 0] == 1.6e308
    W = np.full((2, 5), -7.0)
    for bad_bw, bad_t in ((with_value(bw, (1, 2), -1.0), t), (np.ones((2, 3)), big), (bw, with_value(t, (0, 0), np.nan))):
        x, y = np.ascontiguousarray(bad_bw), np.ascontiguousarray(bad_t)
        assert lib.colate_bootstrap_rows_host(2, 3, 5, x.ctypes.data, y.ctypes.data, W.ctypes.data) == -1
        assert (W == -7.0).all()
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, np.linspace(0, 1, 1025), device=False)
    assert e.value.code == -4
    with pytest.raises(colate_amd.ColateError):
        colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, init, device=False, math=2)


def test_rows_file_rule_in_python_is_what_the_test_means():
    k, a0, a1, t = bl.tables_of()
    assert t.shape == (3, 7) and set(k) == {0, 1} and (a0 == a1).any() and (a1 > 1e8 / 28).any()
    assert t[1, 0] == 2.375 and (t == 0.0).any()  # the repeated cell of block 40, summed


@pytest.mark.parametrize("gz", (False, True))
def test_cli_on_the_host_twin_matches_the_python_composition_byte_for_byte(tmp_path, gz):
    rows = tmp_path / ("rows.txt.gz" if gz else "rows.txt")
    if gz:
        with gzip.open(rows, "wt") as f:
            f.write(bl.rows_text())
    else:
        rows.write_text(bl.rows_text())
    B, seed = 5, 11
    r = bl.run_cli(["--rows", rows, "--bins", "3,7,0.2", "-o", tmp_path / "cli", "--num_bootstraps", B, "--seed", seed], tmp_path,
                   device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "interval fit on the host (COLATE_DEVICE_INTERVAL=0)" in r.stderr
    assert "Number of blocks: 3" in r.stderr and "Number of rows: 7" in r.stderr
    k, a0, a1, t = bl.tables_of()
    ep, ep_null = colate_amd.epochs_from_bins("3,7,0.2")
    rates, iters = bl.composed_coal(tmp_path / "py.coal", k, a0, a1, t, ep, None, ep_null, B, seed)
    assert (tmp_path / "cli.coal").read_bytes() == (tmp_path / "py.coal").read_bytes()
    assert np.unique(rates, axis=0).shape[0] == B and (iters > 1000).all()  # (replicates differ; the defaults of `mut`)
    for i in range(B):
        assert f"Bootstrap {i + 1}: Total iterations {iters[i]}\n" in r.stderr


def test_cli_one_replicate_years_per_gen_and_iteration_limits(tmp_path):
    (tmp_path / "rows.txt").write_text(bl.rows_text())
    r = bl.run_cli(["--rows", "rows.txt", "--bins", "3,7,0.5", "--years_per_gen", "25", "-o", "one", "--max_iter", "30", "--min_iter", "5"],
                   tmp_path, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    k, a0, a1, t = bl.tables_of()
    ep, ep_null = colate_amd.epochs_from_bins("3,7,0.5", 0.0, 25.0)
    rates, iters = bl.composed_coal(tmp_path / "py.coal", k, a0, a1, t, ep, None, ep_null, 1, 12345, max_iter=30, min_iter=5)
    assert (tmp_path / "one.coal").read_bytes() == (tmp_path / "py.coal").read_bytes()
    assert fl.same_bits(colate_amd.bootstrap_weights(colate_amd.Rng(1), 1, 3), np.ones((1, 3)))  # (B = 1: no draw, any seed)


def test_cli_with_coal_takes_the_starting_rates_from_the_file(tmp_path):
    (tmp_path / "rows.txt").write_text(bl.rows_text())
    ep0 = np.unique(colate_amd.epochs_from_bins("3,7,0.4")[0])  # (a .coal file's epochs increase strictly)
    start = np.exp(np.random.default_rng(3).uniform(np.log(1e-6), np.log(1e-3), (1, ep0.size)))
    colate_amd.write_coal(tmp_path / "start.coal", ep0, start)
    args = ["--rows", "rows.txt", "-o", "warm", "--num_bootstraps", 3, "--seed", 4, "--max_iter", 40, "--min_iter", 5]
    r = bl.run_cli(args + ["--coal", "start.coal"], tmp_path, device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    ep, init = colate_amd.epochs_from_coal(tmp_path / "start.coal")
    assert ep.size == ep0.size and not np.allclose(init, colate_amd.DEFAULT_INIT_RATE)
    k, a0, a1, t = bl.tables_of()
    bl.composed_coal(tmp_path / "py.coal", k, a0, a1, t, ep, init, 0, 3, 4, max_iter=40, min_iter=5)
    assert (tmp_path / "warm.coal").read_bytes() == (tmp_path / "py.coal").read_bytes()
    bl.composed_coal(tmp_path / "cold.coal", k, a0, a1, t, ep, None, 0, 3, 4, max_iter=40, min_iter=5)
    assert (tmp_path / "warm.coal").read_bytes() != (tmp_path / "cold.coal").read_bytes()  # (40 iterations: the start shows)


GOOD = "7 shared 1 2 1\n# comment\n"  # lines 1 and 2; the case's line is line 3


@pytest.mark.parametrize("line, what", [
    ("7 shared 1 2", "fields"),
    ("7 shared 1 2 1 9", "fields"),
    ("7 both 1 2 1", "unknown kind"),
    ("-7 shared 1 2 1", "block"),
    ("7.5 shared 1 2 1", "block"),
    ("x shared 1 2 1", "block"),
    ("7 shared 3 2 1", "age_begin"),          # age_begin > age_end
    ("7 shared -1 2 1", "negative age"),
    ("7 shared 1 inf 1", "infinite age"),
    ("7 shared nan nan 1", "age"),
    ("7 shared 1 2x 1", "age_end"),
    ("7 shared 1 2 -1", "weight"),
    ("7 shared 1 2 inf", "weight"),
    ("7 shared 1 2 nan", "weight"),
    ("7 shared 1 2 w", "weight"),
])
def test_cli_errors_name_the_line_and_write_nothing(tmp_path, line, what):
    (tmp_path / "rows.txt").write_text(GOOD + line + "\n7 shared 1 2 1\n")
    r = bl.run_cli(["--rows", "rows.txt", "--bins", "3,7,0.2", "-o", "out"], tmp_path, device=False)
    assert r.returncode == 1
    assert "rows.txt, line 3: " in r.stderr and what in r.stderr, r.stderr[-800:]
    assert not (tmp_path / "out.coal").exists()


def test_cli_empty_and_missing_files_and_missing_arguments(tmp_path):
    (tmp_path / "empty.txt").write_text("# nothing\n\n   \n")
    for args, what in ((["--rows", "empty.txt", "--bins", "3,7,0.2", "-o", "out"], "no rows"),
                       (["--rows", "nowhere.txt", "--bins", "3,7,0.2", "-o", "out"], "cannot open"),
                       (["--rows", "empty.txt", "-o", "out"], "needs --rows"),
                       (["--bins", "3,7,0.2", "-o", "out"], "needs --rows"),
                       (["--rows", "empty.txt", "--bins", "3,7", "-o", "out"], "epochs format"),
                       (["--rows", "empty.txt", "--bins", "3,7,0.2", "-o", "out", "--num_bootstraps", "0"], "at least 1")):
        r = bl.run_cli(args, tmp_path, device=False)
        assert r.returncode == 1 and what in r.stderr, (args, r.stderr[-800:])
        assert not (tmp_path / "out.coal").exists()
