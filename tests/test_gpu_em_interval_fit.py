"""The EM fit on interval-dated mutations on the device (colate_em_interval_batch, csrc/em_interval_fit_kernel.hip): rates,
iteration counts, log-likelihoods and flags bit for bit those of the host twin that runs the same source with the same
exp / log (math=1; em_math.hpp is device = host bit for bit, tests/test_gpu_em_math.py), and within the fixture's bound of
the reference's own fits (tests/golden/l2_interval_fit).  max_iter <= 200 everywhere."""
import numpy as np
import pytest

import colate_amd
import em_interval_fit_lib as fl

pytestmark = pytest.mark.gpu
WAVES = colate_amd.em_interval_batch_waves(23)


def both(k, a0, a1, w, ep, init, max_iter, min_iter, rel_tol, what=""):
    assert max_iter <= 200
    dev = colate_amd.em_interval_batch(k, a0, a1, w, ep, init, max_iter, min_iter, rel_tol)
    host = colate_amd.em_interval_batch(k, a0, a1, w, ep, init, max_iter, min_iter, rel_tol, device=False, math=1)
    fl.assert_same_fit(dev, host, what)
    return host


def test_layouts():
    assert WAVES >= 2 and colate_amd.em_interval_batch_waves(256) == WAVES and colate_amd.em_interval_batch_waves(257) == 1


@pytest.mark.parametrize("E", (2, 23, 64, 65, 256))
def test_epoch_counts_and_row_counts_around_a_group(E):
    """E = 64 / 65: where the lane stride wraps; R = 1, WAVES - 1, WAVES + 1, 2 WAVES + 3: a group that is not full, one
    row in the second group, three groups"""
    for R in (1, WAVES - 1, WAVES + 1, 2 * WAVES + 3):
        k, a0, a1, w, ep, init = fl.random_problem(E, R, 3, seed=100 * E + R, zero_rate_at=E // 3)
        both(k, a0, a1, w, ep, init, 10 if E < 256 else 4, 2, 1e-3, (E, R))


@pytest.mark.parametrize("E", (257, 1024))
def test_one_wave_layout(E):
    k, a0, a1, w, ep, init = fl.random_problem(E, 3, 2, seed=E)
    both(k, a0, a1, w, ep, init, 4, 1, 1e-3, E)


def test_rows_beyond_those_kept_in_registers():
    """a wave keeps its first 64 rows in registers and reads later ones again: R > 64 WAVES, and R > 64 in the one-wave layout"""
    k, a0, a1, w, ep, init = fl.random_problem(8, 64 * WAVES + 5, 2, seed=7)
    w[:, 8:-9] *= (np.arange(w.shape[1] - 17) % 5 == 0)  # (most rows without weight: their groups are skipped)
    both(k, a0, a1, w, ep, init, 3, 1, 1e-3, "multi-wave")
    k, a0, a1, w, ep, init = fl.random_problem(257, 67, 1, seed=8)
    w[:, 2:-3] = 0.0
    both(k, a0, a1, w, ep, init, 2, 0, 1e-3, "one wave")


def test_weights_zero_on_a_group_and_on_a_replicate():
    k, a0, a1, w, ep, init = fl.random_problem(23, 3 * WAVES + 2, 3, seed=11)
    w[0, WAVES:2 * WAVES] = 0.0  # a whole group of rows
    w[1] = 0.0                   # a replicate without data
    w[2, :WAVES] = 0.0
    w[2, WAVES + 1] = 2.0
    host = both(k, a0, a1, w, ep, init, 12, 2, 1e-4)
    assert (host[0][1] == 0.0).all() and host[1][1] == 12 and host[3][1] == colate_amd.api.FLAG_MAXITER


def test_replicates_end_by_the_stop_rule_in_different_iterations():
    c = fl.case("seed2")
    host = fl.fit(c, device=False, math=1)
    assert (host[1] < c["max_iter"]).all() and np.unique(host[1]).size == 3 and (host[3] == 0).all()  # (so it is for these inputs)
    fl.assert_same_fit(fl.fit(c), host)


def test_more_workgroups_than_compute_units():
    k, a0, a1, _, ep, init = fl.random_problem(8, 5, 1, seed=21)
    w = np.random.default_rng(22).integers(0, 4, (300, 5)).astype(float)
    host = both(k, a0, a1, w, ep, init, 12, 3, 1e-3)
    assert np.unique(host[0], axis=0).shape[0] > 100


@pytest.mark.parametrize("name", fl.CASES)
def test_fixture_cases_within_the_bound_of_the_reference(name):
    c = fl.case(name)
    assert c["max_iter"] <= 200
    rates, iters, ll, flags = fl.fit(c)
    fl.check_against_fixture(c, rates, iters)
    assert np.array_equal(flags, np.where(c["iters"] == c["max_iter"], colate_amd.api.FLAG_MAXITER, 0))


def test_no_state_is_left_between_calls():
    k, a0, a1, w, ep, init = fl.random_problem(23, WAVES + 3, 5, seed=31)
    first = colate_amd.em_interval_batch(k, a0, a1, w, ep, init, 8, 2, 1e-4)
    k2, a02, a12, w2, ep2, init2 = fl.random_problem(40, 4, 2, seed=32)
    second = colate_amd.em_interval_batch(k2, a02, a12, w2, ep2, init2, 8, 2, 1e-4)
    colate_amd.api.lib.colate_release_workspace()
    fresh = colate_amd.em_interval_batch(k2, a02, a12, w2, ep2, init2, 8, 2, 1e-4)
    fl.assert_same_fit(second, fresh)
    fl.assert_same_fit(first, colate_amd.em_interval_batch(k, a0, a1, w, ep, init, 8, 2, 1e-4))
