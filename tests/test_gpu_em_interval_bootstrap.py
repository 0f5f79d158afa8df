"""The block bootstrap in front of the interval-dated EM fit on the device (colate_bootstrap_em_interval_batch:
bootstrap_rows_kernel, then em_interval_fit_kernel on the sums it left in device memory): rates, log-likelihoods,
iteration counts and flags bit for bit those of the host twin with the kernels' exp / log (math=1), and `Colate --mode
mut_interval` on the device against the same run on the host twin.  max_iter <= 60, min_iter <= 20 everywhere."""
import numpy as np
import pytest

import colate_amd
import em_interval_bootstrap_lib as bl
import em_interval_fit_lib as fl

pytestmark = pytest.mark.gpu
WAVES = colate_amd.em_interval_batch_waves(23)


def both(k, a0, a1, bw, t, ep, init, max_iter, min_iter, rel_tol, what=""):
    assert max_iter <= 60 and min_iter <= 20
    dev = colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, init, max_iter, min_iter, rel_tol)
    host = colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, init, max_iter, min_iter, rel_tol, device=False, math=1)
    fl.assert_same_fit(dev, host, what)
    return host


@pytest.mark.parametrize("B, nb, R, E", [
    (1, 1, 1, 23),               # one thread of the bootstrap kernel at work
    (5, 7, 9, 23),               # one row past a group of eight
    (3, 4, 64 * WAVES + 3, 23),  # rows beyond those the fit keeps in registers; three workgroups of the bootstrap kernel per replicate
    (2, 3, 17, 300),             # one wave per workgroup of the fit
])
def test_device_equals_the_host_twin_in_every_bit(B, nb, R, E):
    assert (colate_amd.em_interval_batch_waves(E) == 1) == (E == 300)
    k, a0, a1, bw, t, ep, init = bl.random_tables(E, R, B, nb, seed=1000 * E + R)
    host = both(k, a0, a1, bw, t, ep, init, 20 if R < 100 and E < 100 else 6, 3, 1e-4, (B, nb, R, E))
    assert np.isfinite(host[0]).all() and (host[3] & 3 == 0).all()
    if B > 1 and nb > 1:
        assert np.unique(host[0], axis=0).shape[0] > 1  # (the replicates' weights differ, and so do their fits)


def test_a_row_without_weight_and_a_replicate_without_weight():
    k, a0, a1, bw, t, ep, init = bl.random_tables(23, WAVES + 3, 3, 4, seed=77)
    t[:, 2] = 0.0
    t[1, 2] = 3.0            # row 2 is seen in block 1 only
    bw[0] = (2, 0, 1, 1)     # replicate 0 did not draw block 1: its row 2 has weight zero
    bw[1] = 0.0              # replicate 1 drew nothing
    bw[2] = (0, 4, 0, 0)     # replicate 2 drew block 1 alone
    W = colate_amd.bootstrap_rows(bw, t)
    assert W[0, 2] == 0.0 and W[0].sum() > 0 and (W[1] == 0.0).all() and W[2, 2] == 12.0
    host = both(k, a0, a1, bw, t, ep, init, 12, 2, 1e-4)
    assert (host[0][1] == 0.0).all() and host[1][1] == 12 and host[3][1] == colate_amd.api.FLAG_MAXITER
    # the device call is the fit on the sums, as on the host
    fl.assert_same_fit(colate_amd.bootstrap_em_interval_batch(k, a0, a1, bw, t, ep, init, 12, 2, 1e-4),
                       colate_amd.em_interval_batch(k, a0, a1, W, ep, init, 12, 2, 1e-4))


def test_cli_on_the_device_writes_the_bytes_of_the_host_twin(tmp_path):
    (tmp_path / "rows.txt").write_text(bl.rows_text())
    args = ["--rows", "rows.txt", "--bins", "3,7,0.2", "--num_bootstraps", 6, "--seed", 3, "--max_iter", 60, "--min_iter", 20]
    host = bl.run_cli(args + ["-o", "host"], tmp_path, device=False)
    dev = bl.run_cli(args + ["-o", "dev"], tmp_path, device=True)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-1500:], dev.stderr[-1500:])
    assert "interval fit on the host" in host.stderr and "interval fit on the host" not in dev.stderr
    assert (tmp_path / "dev.coal").read_bytes() == (tmp_path / "host.coal").read_bytes()
    assert [x for x in dev.stderr.splitlines() if x.startswith("Bootstrap")] == [x for x in host.stderr.splitlines() if x.startswith("Bootstrap")]
