"""What the interval-dated E-step tests share: the committed reference vectors (tests/golden/l1_interval, made by
tests/golden/make_golden_interval.py) and the tolerances of the single-call checks."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_interval", os.path.join(HERE, "golden", "make_golden_interval.py"))
golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(golden)
RATE_SETS = golden.RATE_SETS


def outside_tolerance(ll, num, den, ll0, num0, den0, ep):
    """per call: True where (ll, num, den) misses (ll0, num0, den0) by more than the single-call tolerances of
    tests/test_gpu_coal_em_shim.py:35-38 -- logl 1e-12 max(1, |ll|), num 1e-8 relative, denom 1e-6 relative + 1e-13 x epoch length"""
    dt = np.append(np.diff(ep), 0.0)
    bad_ll = np.abs(ll - ll0) > 1e-12 * np.maximum(1.0, np.abs(ll0))
    bad_num = (np.abs(num - num0) > 1e-8 * np.abs(num0) + 1e-300).any(axis=1)
    bad_den = (np.abs(den - den0) > 1e-6 * np.abs(den0) + 1e-13 * dt + 1e-300).any(axis=1)
    return bad_ll | bad_num | bad_den


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
