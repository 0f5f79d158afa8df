"""The EM fit on interval-dated mutations (colate_em_interval_batch) on the CPU: its two host twins
(colate_em_interval_batch_host: the loop over csrc/em_interval.hpp with M-step and stop rule of csrc/em_interval_fit.hpp;
math=0 <cmath>, math=1 em_math) against the reference's calls in a loop -- directly where oracle/_ref/libref_em.so has
been built, and through the committed fits (tests/golden/l2_interval_fit) everywhere -- against the oracle of the
point-dated EM, and against a loop over colate_em_interval_calls."""
import ctypes
import json
import os

import numpy as np
import pytest

import colate_amd
import em_interval_fit_lib as fl
import oracle_lib as ol

needs_ref = pytest.mark.skipif(ol.REF is None, reason="oracle/_ref/libref_em.so not built (the reference is not on this machine)")


@needs_ref
@pytest.mark.parametrize("name", fl.CASES)
def test_libm_twin_equals_a_fresh_reference_loop_bit_for_bit(name):
    c = fl.case(name)
    rates0, iters0, ll0 = fl.golden.reference_case(name)
    rates, iters, ll, flags = fl.fit(c, device=False, math=0)
    assert np.array_equal(iters, iters0) and fl.same_bits(rates, rates0) and fl.same_bits(ll, ll0)
    assert np.array_equal(flags & 3, np.zeros_like(flags))


@needs_ref
@pytest.mark.parametrize("name", fl.CASES)
def test_committed_fits_equal_a_fresh_run_of_the_generator(name):
    committed = json.load(open(os.path.join(fl.golden.OUT, name + ".json")))
    fresh, rel = fl.golden.build_case(name)
    assert committed == fresh
    assert rel <= fl.golden.load_meta()["em_math_max_rel_diff"]


@pytest.mark.parametrize("name", fl.CASES)
def test_libm_twin_equals_committed_fits_bit_for_bit(name):
    c = fl.case(name)
    assert c["kinds"].size >= 50 and c["weights"].shape[0] == 3 and (c["weights"] == 0).any()
    assert (c["age_begin"] == c["age_end"]).any() and (c["age_end"] > c["epochs"][-1]).any()
    rates, iters, ll, flags = fl.fit(c, device=False, math=0)
    assert np.array_equal(iters, c["iters"]) and fl.same_bits(rates, c["rates"]) and fl.same_bits(ll, c["loglik"])
    assert np.array_equal(flags, np.where(c["iters"] == c["max_iter"], colate_amd.api.FLAG_MAXITER, 0))


def test_fixture_replicates_end_by_the_stop_rule_in_different_iterations():
    for name in fl.CASES:
        c = fl.case(name)
        assert (c["iters"] < c["max_iter"]).any() and np.unique(c["iters"]).size > 1
        assert c["max_iter"] <= 200


def test_point_rows_from_count_tables_equal_the_point_oracle_bit_for_bit():
    """rows = the age grid's bins ascending, shared before not-shared, weights = the counts: the loop of the point-dated EM,
    which tests/test_oracle_golden.py pins to the reference and the .coal fixtures to its output"""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    csh, cns = workloads.bootstrap_tables(grid, 2, nb=9, scale=1.0)
    csh[:, ::5] = 0.0
    cns[:, 3::7] = 0.0
    kinds = np.tile([0, 1], grid.size)
    ages = np.repeat(grid, 2)
    w = np.stack([csh, cns], axis=2).reshape(csh.shape[0], -1)  # [B][bin][kind]
    for max_iter, min_iter, tol in ((150, 10, 1e-4), (40, 1000, 1e-7)):
        r0, it0, ll0, f0 = ol.em_batch(grid, csh, cns, ep, max_iter=max_iter, min_iter=min_iter, rel_tol=tol)
        rates, iters, ll, flags = colate_amd.em_interval_batch(kinds, ages, ages, w, ep, None, max_iter, min_iter, tol, device=False, math=0)
        assert np.array_equal(iters, it0), (iters, it0)
        assert fl.same_bits(rates, r0) and fl.same_bits(ll, ll0) and np.array_equal(flags, f0)
    assert (it0 == 40).all() and (flags == colate_amd.api.FLAG_MAXITER).all()


@pytest.mark.parametrize("name", fl.CASES)
def test_em_math_twin_within_the_bound_of_the_fixture(name):
    """equal iteration counts, rates within 10 x em_math_max_rel_diff (read from case.json)"""
    c = fl.case(name)
    rates, iters, ll, flags = fl.fit(c, device=False, math=1)
    fl.check_against_fixture(c, rates, iters)


@pytest.mark.parametrize("math", (0, 1))
def test_a_host_loop_over_the_calls_reproduces_the_twin(math):
    """what a caller had to write before: em_interval_calls per iteration, then M-step (the oracle's) and stop rule"""
    c = fl.case("seed2")
    ep, E = c["epochs"], c["epochs"].size
    rates0, iters0, ll0, _ = fl.fit(c, device=False, math=math)
    for b in range(c["weights"].shape[0]):
        rates = c["init_rates"].copy()
        ll, it = -np.inf, 0
        with np.errstate(all="ignore"):
            while it < c["max_iter"]:
                prev = ll
                *_, nacc, dacc, ll = colate_amd.em_interval_calls(c["kinds"], c["age_begin"], c["age_end"], ep, rates,
                                                                  weights=c["weights"][b], device=False, math=math)
                ol.O.oracle_mstep(E, ol.P(nacc), ol.P(dacc), c["rate_floor"], ol.P(rates))
                if (np.float64(ll) / np.float64(prev) > 1.0 - c["rel_tol"]) and it > c["min_iter"]:
                    break
                it += 1
        assert it == iters0[b] and fl.same_bits(rates, rates0[b]) and fl.same_bits(ll, ll0[b]), b


def test_refusals_leave_the_outputs_alone():
    k, a0, a1, w, ep, init = fl.random_problem(8, 5, 2, seed=1)
    good = dict(B=2, R=5, E=8, kinds=k, a0=a0, a1=a1, w=w, ep=ep, init=init, max_iter=10, min_iter=0, rel_tol=1e-6, floor=5e-9)

    def refused(**change):
        a = dict(good, **change)
        for host in (True, False):  # (the checks come before a device is asked for)
            rates, iters = np.full((2, 8), -7.0), np.full(2, -7, dtype=np.int32)
            ll, flags = np.full(2, -7.0), np.full(2, -7, dtype=np.int32)
            arr = [np.ascontiguousarray(a[n], dtype=t) for n, t in (("kinds", np.int32), ("a0", float), ("a1", float), ("w", float),
                                                                     ("ep", float), ("init", float))]
            args = [a["B"], a["R"], a["E"]] + [x.ctypes.data for x in arr] + [a["max_iter"], a["min_iter"], a["rel_tol"], a["floor"],
                                                                              rates.ctypes.data, iters.ctypes.data, ll.ctypes.data, flags.ctypes.data]
            lib = colate_amd.api.lib
            rc = lib.colate_em_interval_batch_host(*args, 0) if host else lib.colate_em_interval_batch(*args)
            assert rc == -1, (change.keys(), rc)
            assert lib.colate_last_error()
            assert (rates == -7.0).all() and (iters == -7).all() and (ll == -7.0).all() and (flags == -7).all()

    def with_value(x, idx, v):
        y = np.array(x, dtype=float)
        y[idx] = v
        return y

    refused(B=0)
    refused(R=0)
    refused(w=with_value(w, (1, 2), -1.0))
    refused(w=with_value(w, (0, 4), np.inf))
    refused(w=with_value(w, (0, 0), np.nan))
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
    refused(a0=with_value(a0, 1, a1[1] * 2))  # (the checks of the calls: age_begin > age_end)
    refused(kinds=np.array([0, 1, 2, 0, 1]))
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.em_interval_batch(k, a0, a1, w, np.linspace(0, 1, 1025), device=False)
    assert e.value.code == -4
    with pytest.raises(colate_amd.ColateError):
        colate_amd.em_interval_batch(k, a0, a1, w, ep, init, device=False, math=2)


def test_edge_replicates():
    k, a0, a1, w, ep, init = fl.random_problem(8, 6, 3, seed=2)
    MAXITER = colate_amd.api.FLAG_MAXITER
    for math in (0, 1):
        # a replicate without data: no row is called, every numerator is 0, every rate becomes 0; only the cap ends it
        w0 = w.copy()
        w0[1] = 0.0
        rates, iters, ll, flags = colate_amd.em_interval_batch(k, a0, a1, w0, ep, init, 12, 2, 1e-6, device=False, math=math)
        assert (rates[1] == 0.0).all() and iters[1] == 12 and ll[1] == 0.0 and flags[1] == MAXITER
        alone = colate_amd.em_interval_batch(k, a0, a1, w0[[0, 2]], ep, init, 12, 2, 1e-6, device=False, math=math)
        fl.assert_same_fit([x[[0, 2]] for x in (rates, iters, ll, flags)], alone)  # (replicates do not see each other)
        # one row; a 1-D weights is one replicate
        r1 = colate_amd.em_interval_batch(k[:1], a0[:1], a1[:1], [2.0], ep, init, 12, 2, 1e-6, device=False, math=math)
        assert r1[0].shape == (1, 8) and np.isfinite(r1[0]).all() and np.isfinite(r1[2]).all() and (r1[3] & 3 == 0).all()
        # one iteration: the cap ends it ("Total iterations" = 1), rates are one M-step from the start
        r2 = colate_amd.em_interval_batch(k, a0, a1, w, ep, init, 1, 0, 1e-6, device=False, math=math)
        assert (r2[1] == 1).all() and (r2[3] == MAXITER).all()
        *_, nacc, dacc, lls = colate_amd.em_interval_calls(k, a0, a1, ep, init, weights=w[0], device=False, math=math)
        want = init.copy()
        ol.O.oracle_mstep(8, ol.P(nacc), ol.P(dacc), 5e-9, ol.P(want))
        assert fl.same_bits(r2[0][0], want) and r2[2][0] == lls
        # a starting rate of 0 inside an interval (and in the epoch of a point): the calls cope, nothing is flagged NaN
        z = init.copy()
        inside = int(np.searchsorted(ep, a0[1], side="right"))  # an epoch that the interval of row 1 covers or touches
        z[min(inside, 7)] = 0.0
        z[0] = 0.0
        r3 = colate_amd.em_interval_batch(k, a0, a1, w, ep, z, 12, 2, 1e-6, device=False, math=math)
        assert np.isfinite(r3[0]).all() and (r3[3] & 1 == 0).all()
