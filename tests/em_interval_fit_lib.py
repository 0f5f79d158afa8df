"""What the tests of the interval-dated EM fit (colate_em_interval_batch) share: the committed reference fits
(tests/golden/l2_interval_fit, made by tests/golden/make_golden_interval_fit.py), the bound that comes with them, and
small random problems."""
import importlib.util
import os

import numpy as np

import colate_amd
from em_interval_lib import same_bits  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_interval_fit", os.path.join(HERE, "golden", "make_golden_interval_fit.py"))
golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(golden)
CASES = tuple(golden.CASES)
FLOOR = golden.RATE_FLOOR
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = golden.load_case(name)
    return _cache[name]


def fit(c, **kw):
    """em_interval_batch on a fixture case"""
    return colate_amd.em_interval_batch(c["kinds"], c["age_begin"], c["age_end"], c["weights"], c["epochs"], c["init_rates"],
                                        c["max_iter"], c["min_iter"], c["rel_tol"], c["rate_floor"], **kw)


def rate_bound():
    """10 x the largest relative rate difference between the <cmath> and the em_math host twin that the generator measured
    over the fixture's cases: the factor covers a libm that differs by ulps on another machine and the few cases sampled"""
    return 10.0 * golden.load_meta()["em_math_max_rel_diff"]


def check_against_fixture(c, rates, iters):
    """equal iteration counts; rates within rate_bound() of the reference's, rates at the floor (in either) equal or skipped"""
    assert np.array_equal(iters, c["iters"]), (iters, c["iters"])
    off_floor = (rates != c["rate_floor"]) & (c["rates"] != c["rate_floor"])
    rel = np.abs(rates - c["rates"])[off_floor] / np.maximum(np.abs(c["rates"][off_floor]), 1e-300)
    print(f"max rel rate diff vs the reference {rel.max(initial=0.0):.3e}, bound {rate_bound():.3e}")
    assert rel.max(initial=0.0) <= rate_bound(), (float(rel.max()), rate_bound())


def random_problem(E, R, B, seed, zero_rate_at=None):
    """epochs from 0 to 1e8 / 28, rows of both kinds: points, intervals, some into the open last epoch; weights 0 .. 3"""
    rng = np.random.default_rng(seed)
    inner = np.sort(np.exp(rng.uniform(np.log(30.0), np.log(2e6), max(E - 2, 0))))
    ep = np.concatenate([[0.0], inner, [1e8 / 28.0]])[:E] if E > 1 else np.array([0.0])
    a0 = np.exp(rng.uniform(np.log(0.1), np.log(1e6), R))
    a1 = a0 * np.exp(rng.uniform(0.01, 3.0, R))
    a1[::4] = a0[::4]
    if R > 2:
        a1[2] = ep[-1] * 1.5
    k = rng.integers(0, 2, R).astype(np.int32)
    w = rng.integers(0, 4, (B, R)).astype(float)
    w[:, 0] = np.maximum(w[:, 0], 1.0)  # (no replicate without data, unless a test makes one)
    init = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), E))
    if zero_rate_at is not None:
        init[zero_rate_at] = 0.0
    return k, a0, a1, w, ep, init


def assert_same_fit(got, want, what=""):
    for name, g, h in zip(("rates", "iters", "loglik", "flags"), got, want):
        if name in ("iters", "flags"):
            assert np.array_equal(g, h), (what, name, g, h)
        else:
            assert same_bits(g, h), (what, name, g, h)
