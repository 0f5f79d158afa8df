"""Interval-dated mutations in the E-step (coal_EM with age_begin < age_end) on the CPU: the host twins of the kernel
(colate_em_interval_calls_host: csrc/em_interval.hpp with <cmath>, math=0, and with em_math, math=1) against the
reference -- directly where oracle/_ref/libref_em.so has been built, and through the committed vectors everywhere."""
import gzip
import json
import os

import numpy as np
import pytest

import colate_amd
import em_interval_lib as il
import oracle_lib as ol

needs_ref = pytest.mark.skipif(ol.REF is None, reason="oracle/_ref/libref_em.so not built (the reference is not on this machine)")


def _ref(kind, ep, rates, a, b):
    n, d = np.zeros(ep.size), np.zeros(ep.size)
    ll = ol.REF.ref_em_call(int(kind), ep.size, ol.P(ep), ol.P(rates), float(a), float(b), ol.P(n), ol.P(d))
    return ll, n, d


@needs_ref
@pytest.mark.parametrize("name", il.RATE_SETS)
def test_host_twin_equals_reference_bit_for_bit(name):
    """same operations in the same order on the same libm: num, denom and the return value of every call of the grid"""
    ep, rates, calls = il.golden.inputs(name)
    k, a0, a1 = np.array([c[0] for c in calls]), np.array([c[1] for c in calls]), np.array([c[2] for c in calls])
    num, den, ll, flags = colate_amd.em_interval_calls(k, a0, a1, ep, rates, device=False, math=0)
    assert (flags == 0).all()
    differ = []
    for r in range(k.size):
        ll0, n0, d0 = _ref(k[r], ep, rates, a0[r], a1[r])
        if not (il.same_bits(ll[r], ll0) and il.same_bits(num[r], n0) and il.same_bits(den[r], d0)):
            differ.append(r)
    assert not differ, (len(differ), differ[:5])


@needs_ref
def test_host_twin_equals_reference_at_the_edges():
    """ages on epoch boundaries, both ages in one epoch, an interval from 0, a zero rate inside and below the interval, and
    point rows (age_begin == age_end) in every epoch, the open last one included"""
    ep, rates, _ = il.golden.inputs("loguniform_seed1")
    zr = rates.copy()
    zr[[2, 9]] = 0.0
    E = ep.size
    pairs = [(0.0, 1.0), (0.0, float(ep[1])), (float(ep[3]), float(ep[4])), (float(ep[3]), float(ep[7])), (40.0, 41.0),
             (float(ep[5]), float(np.nextafter(ep[5], np.inf))), (float(np.nextafter(ep[6], 0.0)), float(ep[6])),
             (1.0, float(np.nextafter(ep[E - 1], 0.0))), (float(ep[E - 2]), float(ep[E - 2]) * 1.5), (3.0, 3.0), (0.0, 0.0),
             (1.0, float(ep[E - 1])), (50.0, float(ep[E - 1]) * 2.0), (float(ep[E - 1]), float(ep[E - 1]) * 1.5),  # into the open last epoch
             (float(ep[E - 1]) * 1.1, float(ep[E - 1]) * 1.2)]
    pairs += [(float(x), float(x)) for x in ep] + [(float(x) * 1.3 + 1.0, float(x) * 1.3 + 1.0) for x in ep]
    for r_ in (rates, zr):
        for kind in (0, 1):
            k = np.full(len(pairs), kind)
            num, den, ll, _ = colate_amd.em_interval_calls(k, [p[0] for p in pairs], [p[1] for p in pairs], ep, r_, device=False, math=0)
            for i, (a, b) in enumerate(pairs):
                if kind == 1 and not b < ep[E - 1] and not r_[E - 1] > 0:
                    continue  # the reference asserts here
                ll0, n0, d0 = _ref(kind, ep, r_, a, b)
                assert il.same_bits(ll[i], ll0) and il.same_bits(num[i], n0) and il.same_bits(den[i], d0), (kind, a, b)


@needs_ref
@pytest.mark.parametrize("name", il.RATE_SETS)
def test_committed_vectors_equal_a_fresh_run_of_the_reference(name):
    with gzip.open(os.path.join(il.golden.OUT, name + ".json.gz"), "rt") as f:
        committed = json.load(f)
    assert committed == il.golden.build_case(name)
    meta = json.load(open(os.path.join(il.golden.OUT, "case.json")))["rate_sets"][name]
    assert meta["calls"] == len(committed["calls"]) and meta["reference_unstable"] == committed["stable"].count(0)


@pytest.mark.parametrize("name", il.RATE_SETS)
def test_host_twin_equals_committed_vectors_bit_for_bit(name):
    ep, rates, k, a0, a1, ll0, n0, d0, _ = il.golden.load_case(name)
    assert k.size >= 300
    num, den, ll, flags = colate_amd.em_interval_calls(k, a0, a1, ep, rates, device=False, math=0)
    assert (flags == 0).all()
    assert il.same_bits(ll, ll0) and il.same_bits(num, n0) and il.same_bits(den, d0)


@pytest.mark.parametrize("name", il.RATE_SETS)
def test_em_math_twin_within_the_single_call_tolerances(name):
    """the twin the device is bit-identical to (exp / log of em_math.hpp) against the reference's vectors, with the stored mask"""
    ep, rates, k, a0, a1, ll0, n0, d0, stable = il.golden.load_case(name)
    num, den, ll, _ = colate_amd.em_interval_calls(k, a0, a1, ep, rates, device=False, math=1)
    assert (~stable).sum() <= 0.05 * k.size
    bad = il.outside_tolerance(ll, num, den, ll0, n0, d0, ep) & stable
    assert not bad.any(), np.flatnonzero(bad)[:10]


def test_point_rows_equal_the_point_path():
    """age_begin == age_end inside a batch: the oracle's per-bin call (bit for bit the reference, tests/test_oracle_golden.py)"""
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    rng = np.random.default_rng(4)
    rates = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), ep.size))
    rates[4] = 0.0
    grid = ol.age_grid()
    ages = np.concatenate([grid[[0, 1, 30, 41, 64, 65, 90, 120, 150, 170, 184]], ep[[3, 8]], [ep[-1] * 1.01]])
    for kind in (0, 1):
        mixed_a1 = ages.copy()
        mixed_a1[::3] = mixed_a1[::3] * 1.25 + 0.5  # every third row an interval: the point rows do not depend on their neighbours
        mixed_a1[-1] = ages[-1]
        num, den, ll, flags = colate_amd.em_interval_calls(np.full(ages.size, kind), ages, mixed_a1, ep, rates, device=False, math=0)
        for i, a in enumerate(ages):
            if mixed_a1[i] != a:
                continue
            ll0, n0, d0 = ol.em_call(kind, ep, rates, a)
            assert il.same_bits(ll[i], ll0) and il.same_bits(num[i], n0) and il.same_bits(den[i], d0), (kind, a)


def test_weighted_sums_follow_the_row_order():
    ep, rates, k, a0, a1, *_ = il.golden.load_case("loguniform_seed1")
    w = np.random.default_rng(3).integers(0, 4, k.size).astype(float)
    for math in (0, 1):
        num, den, ll, _, nacc, dacc, lls = colate_amd.em_interval_calls(k, a0, a1, ep, rates, weights=w, device=False, math=math)
        n, d, s = np.zeros(ep.size), np.zeros(ep.size), 0.0
        for r in range(k.size):
            if w[r] > 0:
                n, d, s = n + w[r] * num[r], d + w[r] * den[r], s + w[r] * ll[r]
        assert il.same_bits(nacc, n) and il.same_bits(dacc, d) and il.same_bits(lls, s)


def test_refusals():
    ep, rates, _ = il.golden.inputs("const_5e-5")
    last = float(ep[-1])

    def refused(a, b, kind=0, epochs=ep, **kw):
        for dev in (False, True):  # (the checks come before a device is asked for)
            with pytest.raises(colate_amd.ColateError) as e:
                colate_amd.em_interval_calls([kind], [a], [b], epochs, rates, device=dev, **kw)
            assert e.value.code == -1, e.value

    refused(10.0, 5.0)                      # age_begin > age_end
    refused(-1.0, 5.0)                      # a negative age
    refused(-2.0, -2.0)
    refused(5.0, float("inf"))
    refused(float("nan"), 5.0)
    refused(1.0, 2.0, kind=2)
    refused(1.0, 2.0, epochs=ep[::-1].copy())
    refused(1.0, 2.0, epochs=ep + 5.0)      # an age before epochs[0]
    with pytest.raises(colate_amd.ColateError):
        colate_amd.em_interval_calls([0], [1.0], [2.0], ep, rates, device=False, math=2)
    # the open last epoch is not refused, for a point or for an interval: the reference's own test grid reaches into it
    num, den, ll, flags = colate_amd.em_interval_calls([0, 1, 0, 1, 1], [last, last * 2, 5.0, 5.0, last], [last, last * 2, last, last * 2, last * 2],
                                                       ep, rates, device=False, math=0)
    assert np.isfinite(num).all() and np.isfinite(den).all() and (flags == 0).all()
