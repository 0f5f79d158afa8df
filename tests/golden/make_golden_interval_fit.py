#!/usr/bin/env python3
"""Generates tests/golden/l2_interval_fit/ from the REFERENCE ITSELF: the EM fit on interval-dated mutations, i.e. the
loop of coal.cpp:3675-3827 (regularise == 2) with rows (kind, age_begin, age_end) for age bins.  The reference wrote and
tested the calls (coal_EM with age_begin < age_end) but has no such loop, so it is driven here: every call is the
reference's own coal_EM through oracle/_ref/libref_em.so (ol.REF.ref_em_call), the sums are those of coal.cpp:3704-3733
with weights for counts, the M-step is oracle_mstep (bit for bit coal.cpp:3771-3815, tests/test_oracle_golden.py) and the
stop test is applied exactly as oracle_em_run applies it.  Runs only where the reference has been built
(make -C oracle ref) and the library too (the two host twins are consulted for the refusals below).

Cases: --bins 3,7,0.2 (23 epochs); 60 rows drawn from the bin1 <= bin2 pairs of the 185-point age grid, both kinds --
point rows, intervals inside one epoch, intervals reaching into the open last epoch, the rest random; B = 3 weight rows
of integers 0 .. 3 (zeros among them); min_iter, max_iter, rel_tol such that replicates end by the stop rule, and not in
the same iteration.

A case is REFUSED (the generator stops) if two runs of the reference loop differ, if the reference asserts on it
(coal.cpp:3711-3714: a NaN or negative sufficient statistic; coal_EM.cpp:351: a not-shared age in the last epoch at rate
0 -- checked here before the call, the reference would abort the process), or if the <cmath> and em_math host twins of
colate_em_interval_batch end any replicate in different iterations.

Per case one <name>.json: inputs, and per replicate rates, iterations, log-likelihood (hex floats, bit-exact).  case.json
records `em_math_max_rel_diff`: the largest relative rate difference between the two twins over all cases, rates at
the floor left out -- the unit of the bound under which the em_math twin and the device are held to these vectors.
    python tests/golden/make_golden_interval_fit.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "l2_interval_fit")
BINS = "3,7,0.2"
RATE_FLOOR = 5e-9
# name: (seed, min_iter, max_iter, rel_tol)
CASES = {"seed1": (1, 20, 200, 1e-4), "seed2": (2, 5, 200, 1e-5), "seed3_cap": (3, 30, 120, 1e-5)}
ROWS, B = 60, 3


class CaseRefused(Exception):
    pass


def hexes(a):
    return [float(x).hex() for x in np.atleast_1d(a)]


def inputs(name):
    """-> (epochs, kinds, age_begin, age_end, weights[B][ROWS], init_rates, min_iter, max_iter, rel_tol)"""
    import oracle_lib as ol

    seed, min_iter, max_iter, rel_tol = CASES[name]
    rng = np.random.default_rng(seed)
    ep, _ = ol.epochs_from_bins(BINS)
    grid = ol.age_grid()
    epoch_of = np.searchsorted(ep, grid, side="right") - 1
    same_epoch = [(b, b + 1) for b in range(grid.size - 1) if epoch_of[b] == epoch_of[b + 1] and epoch_of[b] < ep.size - 1]
    in_last = np.flatnonzero(epoch_of == ep.size - 1)
    pairs = []
    pairs += [(b, b) for b in rng.choice(grid.size, 12, replace=False)]                      # point rows
    pairs += [(int(in_last[0]), int(in_last[0]))]                                            # a point in the open last epoch
    pairs += [same_epoch[i] for i in rng.choice(len(same_epoch), 8, replace=False)]          # inside one epoch
    pairs += [(int(rng.integers(0, in_last[0])), int(b)) for b in rng.choice(in_last, 8)]    # into the open last epoch
    pairs += [(int(in_last[1]), int(in_last[4]))]                                            # both ages in it
    while len(pairs) < ROWS:
        b1, b2 = sorted(int(x) for x in rng.integers(0, grid.size, 2))
        pairs.append((b1, b2))
    order = rng.permutation(ROWS)
    pairs = [pairs[i] for i in order]
    kinds = rng.integers(0, 2, ROWS).astype(np.int32)
    a0 = np.array([grid[p[0]] for p in pairs])
    a1 = np.array([grid[p[1]] for p in pairs])
    weights = rng.integers(0, 4, (B, ROWS)).astype(float)
    init = np.full(ep.size, 1.0 / 20000.0)
    return ep, kinds, a0, a1, weights, init, min_iter, max_iter, rel_tol


def reference_fit(ep, kinds, a0, a1, w, init, min_iter, max_iter, rel_tol, rate_floor=RATE_FLOOR):
    """one replicate (w[ROWS]) through the reference's calls -> (rates, iterations, loglik)"""
    import oracle_lib as ol

    assert ol.REF is not None, "oracle/_ref/libref_em.so missing: make -C oracle ref"
    E = ep.size
    rates = np.array(init, dtype=np.float64)
    num, den = np.zeros(E), np.zeros(E)
    ll = prev_ll = -np.inf
    it = 0
    with np.errstate(all="ignore"):
        while it < max_iter:
            prev_ll = ll
            num_acc, den_acc, ll = np.zeros(E), np.zeros(E), np.float64(0.0)
            for r in range(kinds.size):
                if not w[r] > 0:
                    continue
                if kinds[r] == 1 and not a1[r] < ep[E - 1] and not rates[E - 1] > 0:
                    raise CaseRefused(f"coal_EM.cpp:351 would assert (row {r}, iteration {it})")
                logl = ol.REF.ref_em_call(int(kinds[r]), E, ol.P(ep), ol.P(rates), float(a0[r]), float(a1[r]), ol.P(num), ol.P(den))
                if np.isnan(num).any() or np.isnan(den).any() or (num < 0).any() or (den < 0).any():
                    raise CaseRefused(f"coal.cpp:3711-3714 would assert (row {r}, iteration {it})")
                ll = ll + np.float64(w[r]) * np.float64(logl)
                num_acc += w[r] * num
                den_acc += w[r] * den
            ol.O.oracle_mstep(E, ol.P(num_acc), ol.P(den_acc), rate_floor, ol.P(rates))
            if (np.float64(ll) / np.float64(prev_ll) > 1.0 - rel_tol) & (it > min_iter):  # coal.cpp:3822, as oracle_em_run
                break
            it += 1
    return rates, it, float(ll)


def reference_case(name):
    ep, kinds, a0, a1, weights, init, min_iter, max_iter, rel_tol = inputs(name)
    fits = [reference_fit(ep, kinds, a0, a1, weights[b], init, min_iter, max_iter, rel_tol) for b in range(weights.shape[0])]
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits], dtype=np.int32), np.array([f[2] for f in fits])


def build_case(name):
    """-> (the case as stored, largest relative rate difference between the two host twins off the floor)"""
    import colate_amd

    ep, kinds, a0, a1, weights, init, min_iter, max_iter, rel_tol = inputs(name)
    rates, iters, ll = reference_case(name)
    again = reference_case(name)
    if not (np.array_equal(rates.view(np.uint64), again[0].view(np.uint64)) and np.array_equal(iters, again[1])
            and np.array_equal(ll.view(np.uint64), again[2].view(np.uint64))):
        raise CaseRefused(f"{name}: two runs of the reference loop differ")
    twins = [colate_amd.em_interval_batch(kinds, a0, a1, weights, ep, init, max_iter, min_iter, rel_tol, RATE_FLOOR, device=False, math=m)
             for m in (0, 1)]
    if not np.array_equal(twins[0][1], twins[1][1]):
        raise CaseRefused(f"{name}: the two host twins end in different iterations: {twins[0][1]} / {twins[1][1]}")
    if not ((iters < max_iter).any() and np.unique(iters).size > 1):
        raise CaseRefused(f"{name}: iterations {iters}: no replicate ends by the stop rule, or all end together")
    off_floor = (twins[0][0] != RATE_FLOOR) & (twins[1][0] != RATE_FLOOR)
    r0, r1 = twins[0][0][off_floor], twins[1][0][off_floor]
    rel = np.abs(r1 - r0)[r1 != r0] / np.abs(r0[r1 != r0])  # (equal rates, zeros among them, differ by 0)
    case = {"generator": "tests/golden/make_golden_interval_fit.py (oracle/_ref/libref_em.so)", "bins": BINS, "epochs": hexes(ep),
            "kinds": [int(k) for k in kinds], "age_begin": hexes(a0), "age_end": hexes(a1), "weights": [hexes(row) for row in weights],
            "init_rates": hexes(init), "min_iter": min_iter, "max_iter": max_iter, "rel_tol": float(rel_tol).hex(),
            "rate_floor": float(RATE_FLOOR).hex(), "rates": [hexes(row) for row in rates], "iters": [int(i) for i in iters],
            "loglik": hexes(ll)}
    return case, float(rel.max(initial=0.0))


def load_case(name):
    """-> dict of arrays / numbers: epochs, kinds, age_begin, age_end, weights, init_rates, min_iter, max_iter, rel_tol,
    rate_floor, rates, iters, loglik"""
    c = json.load(open(os.path.join(OUT, name + ".json")))
    fh = float.fromhex
    vec = lambda xs: np.array([fh(x) for x in xs])  # noqa: E731
    mat = lambda rows: np.array([[fh(x) for x in row] for row in rows])  # noqa: E731
    return {"epochs": vec(c["epochs"]), "kinds": np.array(c["kinds"], dtype=np.int32), "age_begin": vec(c["age_begin"]),
            "age_end": vec(c["age_end"]), "weights": mat(c["weights"]), "init_rates": vec(c["init_rates"]),
            "min_iter": c["min_iter"], "max_iter": c["max_iter"], "rel_tol": fh(c["rel_tol"]), "rate_floor": fh(c["rate_floor"]),
            "rates": mat(c["rates"]), "iters": np.array(c["iters"], dtype=np.int32), "loglik": vec(c["loglik"])}


def load_meta():
    return json.load(open(os.path.join(OUT, "case.json")))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    os.makedirs(OUT, exist_ok=True)
    meta = {"generator": "tests/golden/make_golden_interval_fit.py (oracle/_ref/libref_em.so)", "cases": {}, "em_math_max_rel_diff": 0.0}
    for name in CASES:
        case, rel = build_case(name)
        json.dump(case, open(os.path.join(OUT, name + ".json"), "w"), indent=0)
        meta["cases"][name] = {"rows": len(case["kinds"]), "iters": case["iters"], "max_iter": case["max_iter"],
                               "em_math_max_rel_diff": rel}
        meta["em_math_max_rel_diff"] = max(meta["em_math_max_rel_diff"], rel)
        print(f"{name}: iterations {case['iters']} (cap {case['max_iter']}), twins differ by at most {rel:.3e} off the floor")
    json.dump(meta, open(os.path.join(OUT, "case.json"), "w"), indent=1)
