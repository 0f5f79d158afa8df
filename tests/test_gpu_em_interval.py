"""Interval-dated mutations in the E-step on the device (colate_em_interval_calls, csrc/em_interval_kernel.hip): bit for
bit the host twin that runs the same source with the same exp / log (em_math.hpp is device = host bit for bit,
tests/test_gpu_em_math.py), and within the single-call tolerances of the reference's own vectors
(tests/golden/l1_interval, with the stability mask that was made from the reference and stored with them)."""
import json
import os
import subprocess

import numpy as np
import pytest

import colate_amd
import em_interval_lib as il

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", il.RATE_SETS)
def test_device_equals_host_twin_bit_for_bit(name):
    ep, rates, k, a0, a1, *_ = il.golden.load_case(name)
    w = np.random.default_rng(5).integers(0, 5, k.size).astype(float)
    dev = colate_amd.em_interval_calls(k, a0, a1, ep, rates, weights=w)
    host = colate_amd.em_interval_calls(k, a0, a1, ep, rates, weights=w, device=False, math=1)
    assert np.array_equal(dev[3], host[3])
    for what, d, h in zip(("num", "denom", "logl", "flags", "num_acc", "den_acc", "ll"), dev, host):
        if what != "flags":
            assert il.same_bits(d, h), what


def test_device_equals_host_twin_on_mixed_rows_and_many_epochs():
    """point rows among interval rows, a zero rate, a batch that does not fill its last workgroup, and E beyond 256 (one
    call per workgroup)"""
    rng = np.random.default_rng(8)
    for E, R in ((24, 37), (300, 9), (1024, 3)):
        ep = np.concatenate([[0.0], np.sort(np.exp(rng.uniform(np.log(30.0), np.log(2e6), E - 2))), [1e8 / 28.0]])
        rates = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), E))
        rates[E // 3] = 0.0
        a0 = np.exp(rng.uniform(np.log(0.1), np.log(1e6), R))
        a1 = a0 * np.exp(rng.uniform(0.01, 3.0, R))  # (some reach into the open last epoch)
        a1[::4] = a0[::4]
        a0[1], a1[1] = ep[5], ep[9]
        k = rng.integers(0, 2, R)
        w = rng.uniform(0.0, 3.0, R)
        dev = colate_amd.em_interval_calls(k, a0, a1, ep, rates, weights=w)
        host = colate_amd.em_interval_calls(k, a0, a1, ep, rates, weights=w, device=False, math=1)
        assert np.array_equal(dev[3], host[3])
        for i in (0, 1, 2, 4, 5, 6):
            assert il.same_bits(dev[i], host[i]), (E, i)


@pytest.mark.parametrize("name", il.RATE_SETS)
def test_device_within_tolerance_of_the_reference_vectors(name):
    """a call is left out only where the reference alone is unstable (the stored mask: one-ulp nudges of its ages move its own
    output beyond these tolerances); at most 5 % of a rate set may be"""
    ep, rates, k, a0, a1, ll0, n0, d0, stable = il.golden.load_case(name)
    meta = json.load(open(os.path.join(il.golden.OUT, "case.json")))
    assert (~stable).sum() == meta["rate_sets"][name]["reference_unstable"]
    assert (~stable).sum() <= 0.05 * k.size
    num, den, ll, flags = colate_amd.em_interval_calls(k, a0, a1, ep, rates)
    assert (flags == 0).all()
    miss = il.outside_tolerance(ll, num, den, ll0, n0, d0, ep)
    print(f"{name}: {k.size} calls, {int((~stable).sum())} masked, {int(miss.sum())} outside tolerance ({int((miss & stable).sum())} unmasked), "
          f"max |dll| {np.abs(ll - ll0).max():.3e}, max num rel {np.max(np.abs(num - n0) / np.maximum(np.abs(n0), 1e-300)):.3e}")
    assert not (miss & stable).any(), np.flatnonzero(miss & stable)[:10]


def test_point_rows_reproduce_the_estep_per_bin():
    ep, _ = colate_amd.epochs_from_bins("3,7,0.2")
    rates = np.exp(np.random.default_rng(4).uniform(np.log(1e-6), np.log(1e-3), ep.size))
    ages = colate_amd.age_grid()[[1, 30, 41, 64, 65, 90, 120, 150, 170, 184]]
    em = colate_amd.coal_EM(ep, rates)
    for kind in (0, 1):
        n0, d0, ll0, _ = em.EM_many(ages, shared=kind == 0)
        num, den, ll, flags = colate_amd.em_interval_calls(np.full(ages.size, kind), ages, ages, ep, rates)
        assert (flags == 0).all()
        assert not il.outside_tolerance(ll, num, den, ll0, n0, d0, ep).any()


def test_coal_EM_takes_intervals():
    ep, rates, k, a0, a1, *_ = il.golden.load_case("const_5e-5")
    em = colate_amd.coal_EM(ep, rates)
    for r in (0, 1, 400, 811):
        num, den = np.zeros(ep.size), np.zeros(ep.size)
        f = em.EM_shared if k[r] == 0 else em.EM_notshared
        ll = f(a0[r], a1[r], num, den)  # (raised NotImplementedError before)
        want = colate_amd.em_interval_calls([k[r]], [a0[r]], [a1[r]], ep, rates)
        assert il.same_bits(num, want[0][0]) and il.same_bits(den, want[1][0]) and ll == want[2][0]
        assert np.isfinite(ll) and (num >= 0).all() and (den >= 0).all() and num.sum() > 0
    with pytest.raises(colate_amd.ColateError):
        em.EM_shared(5.0, 1.0, np.zeros(ep.size), np.zeros(ep.size))


def test_cxx_call_site_on_the_reference_grid():
    """csrc/tools/coal_EM_interval_check.cpp: the second half of the reference's test of the class (E = 21, seven constant
    rates, every bin1 <= bin2 of its 92 ages, both kinds) through include/colate_coal_EM.hpp: every output a number >= 0"""
    exe = os.path.join(ROOT, "colate_amd", "bin", "coal_EM_interval_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 7 * (92 * 93 // 2) * 2
    vals = np.array([[float.fromhex(t) for t in line.split()[4:]] for line in lines])
    assert np.isfinite(vals).all() and (vals[:, 1:] >= 0).all()
