#!/usr/bin/env python3
"""Generates tests/golden/l1_interval/ from the REFERENCE ITSELF: coal_EM::EM_shared / EM_notshared with
age_begin < age_end (coal_EM.cpp:212-242, 359-433) through oracle/_ref/libref_em.so, as make_golden.py does for the
point form.  Runs only where the reference has been built (make -C oracle ref).

Inputs: 24 epochs 0, 10^(3.0 .. 7.0 step 0.2)/28, 10^7.2/28, 1e8/28; ages exp(b/5)/10 below 0.9 x the last boundary,
every third bin, every b1 < b2, both kinds; two rate sets: 5e-5 constant, and log-uniform 1e-6 .. 1e-3
(numpy default_rng(1)).

Per rate set one <name>.json.gz: epochs, rates, calls [kind, age_begin, age_end], and per call logl, num[E], denom[E]
as hex floats (bit-exact), plus `stable`: 0 where the REFERENCE ALONE is unstable -- where moving age_begin or
age_end by one ulp (four nudged calls) changes the reference's own output by more than the tolerances the device is
held to (TOL below: those of the single-call checks, tests/test_gpu_coal_em_shim.py).  The mask is made here, from the
reference, and stored; nothing of the code under test enters it.  case.json records the counts.
    python tests/golden/make_golden_interval.py
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "l1_interval")
RATE_SETS = ("const_5e-5", "loguniform_seed1")
TOL = {"logl_rel": 1e-12, "num_rel": 1e-8, "denom_rel": 1e-6, "denom_abs_per_epoch_length": 1e-13}


def hexes(a):
    return [float(x).hex() for x in np.atleast_1d(a)]


def inputs(name):
    ep = np.concatenate([[0.0], 10.0 ** (3.0 + 0.2 * np.arange(21)) / 28.0, [10.0 ** 7.2 / 28.0, 1e8 / 28.0]])
    E = ep.size
    rates = np.full(E, 5e-5) if name == "const_5e-5" else np.exp(np.random.default_rng(1).uniform(np.log(1e-6), np.log(1e-3), E))
    ages = [a for a in (float(np.exp(b / 5.0) / 10.0) for b in range(0, 92, 3)) if a < 0.9 * ep[-1]]
    calls = [(kind, a, b) for i, a in enumerate(ages) for b in ages[i + 1:] for kind in (0, 1)]
    return ep, rates, calls


def within(ll, num, den, ll0, num0, den0, ep):
    """the tolerances of the single-call checks, around the values (ll0, num0, den0)"""
    dt = np.append(np.diff(ep), 0.0)
    return bool(abs(ll - ll0) <= TOL["logl_rel"] * max(1.0, abs(ll0))
                and (np.abs(num - num0) <= TOL["num_rel"] * np.abs(num0) + 1e-300).all()
                and (np.abs(den - den0) <= TOL["denom_rel"] * np.abs(den0) + TOL["denom_abs_per_epoch_length"] * dt + 1e-300).all())


def build_case(name):
    import oracle_lib as ol

    assert ol.REF is not None, "oracle/_ref/libref_em.so missing: make -C oracle ref"
    ep, rates, calls = inputs(name)
    E = ep.size

    def ref(kind, a, b):
        n, d = np.zeros(E), np.zeros(E)
        ll = ol.REF.ref_em_call(kind, E, ol.P(ep), ol.P(rates), float(a), float(b), ol.P(n), ol.P(d))
        return ll, n, d

    case = {"generator": "tests/golden/make_golden_interval.py (oracle/_ref/libref_em.so)", "epochs": hexes(ep),
            "rates": hexes(rates), "calls": [], "logl": [], "num": [], "denom": [], "stable": []}
    for kind, a, b in calls:
        ll0, n0, d0 = ref(kind, a, b)
        stable = True
        for a2, b2 in ((np.nextafter(a, 0.0), b), (np.nextafter(a, np.inf), b), (a, np.nextafter(b, 0.0)), (a, np.nextafter(b, np.inf))):
            stable = stable and within(*ref(kind, a2, b2), ll0, n0, d0, ep)
        case["calls"].append([kind, float(a).hex(), float(b).hex()])
        case["logl"].append(float(ll0).hex())
        case["num"].append(hexes(n0))
        case["denom"].append(hexes(d0))
        case["stable"].append(int(stable))
    return case


def load_case(name):
    """-> (epochs, rates, kinds, age_begin, age_end, logl, num, denom, stable) as arrays"""
    with gzip.open(os.path.join(OUT, name + ".json.gz"), "rt") as f:
        c = json.load(f)
    fh = float.fromhex
    arr = lambda rows: np.array([[fh(x) for x in row] for row in rows])  # noqa: E731
    return (np.array([fh(x) for x in c["epochs"]]), np.array([fh(x) for x in c["rates"]]),
            np.array([k for k, _, _ in c["calls"]], dtype=np.int32), np.array([fh(a) for _, a, _ in c["calls"]]),
            np.array([fh(b) for _, _, b in c["calls"]]), np.array([fh(x) for x in c["logl"]]), arr(c["num"]), arr(c["denom"]),
            np.array(c["stable"], dtype=bool))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    meta = {"generator": "tests/golden/make_golden_interval.py (oracle/_ref/libref_em.so)", "tolerances": TOL,
            "unstable_cap": 0.05, "rate_sets": {}}
    for name in RATE_SETS:
        case = build_case(name)
        with open(os.path.join(OUT, name + ".json.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as g:
            g.write(json.dumps(case).encode())
        n, unstable = len(case["calls"]), len(case["stable"]) - sum(case["stable"])
        zero_ll = sum(1 for x in case["logl"] if float.fromhex(x) == 0.0)
        meta["rate_sets"][name] = {"calls": n, "reference_unstable": unstable, "reference_failures": zero_ll}
        print(f"{name}: {n} calls, {unstable} where the reference alone is unstable, {zero_ll} reference failures")
    json.dump(meta, open(os.path.join(OUT, "case.json"), "w"), indent=1)
