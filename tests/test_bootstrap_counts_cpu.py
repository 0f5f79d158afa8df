"""CPU: the plain model of the count bootstrap (bootstrap_counts_lib.py) against the oracle's restatement of
coal.cpp:3358-3441, against the host twin of the kernel (colate_bootstrap_counts_from_weights) and against exact
arithmetic, over the whole edge matrix and the groups problem; the cases are what their names say; an age outside the
grid is an error of the host twin.  Every comparison of count tables is bit for bit."""
import ctypes

import numpy as np
import pytest

import bootstrap_counts_lib as bl
import oracle_lib as ol


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    return colate_amd


def _oracle(grid, age, weights, tabs):
    g, t = ol.f64(grid), [ol.f64(x) for x in tabs]
    nb, A = t[0].shape
    csh, cns = np.zeros((len(weights), A)), np.zeros((len(weights), A))
    for i, w in enumerate(weights):
        w = ol.f64(w)
        ol.O.oracle_bootstrap_counts(nb, A, ol.P(g), float(age), ol.P(w), ol.P(t[0]), ol.P(t[1]), ol.P(t[2]), ol.P(t[3]),
                                     ol.P(csh[i]), ol.P(cns[i]))
    return csh, cns


def test_matrix_holds_every_case():
    assert bl.assert_matrix_counts() == 2772
    keys = {c.key for A in bl.A_VALUES for c in bl.matrix_cases(A)}
    assert len(keys) == 2808
    # the only ages of the matrix that fall outside: grid[A//2] at A = 2, where it is the last grid point
    assert {(c.A, c.ai) for c in bl.outside_cases()[:bl.N_MATRIX_OUTSIDE]} == {(2, 2)}


@pytest.mark.parametrize("A", bl.A_VALUES)
def test_model_equals_oracle_and_host_twin(ca, A):
    """Model == oracle == colate_bootstrap_counts_from_weights on every in-grid case of the matrix (the oracle is never
    called with an age outside the grid: its search for bin_start has no bound)."""
    model = bl.matrix_model(A)
    assert len(model) == len(bl.in_grid_cases(A))
    for c in bl.in_grid_cases(A):
        m_sh, m_ns, _ = model[c.key]
        o_sh, o_ns = _oracle(c.grid, c.age, c.weights, c.tabs)
        h_sh, h_ns = ca.bootstrap_counts_from_weights(c.grid, c.age, c.weights, *c.tabs)
        assert np.array_equal(m_sh, o_sh) and np.array_equal(m_ns, o_ns), ("model != oracle", c)
        assert np.array_equal(m_sh, h_sh) and np.array_equal(m_ns, h_ns), ("model != host twin", c)


@pytest.mark.parametrize("grid_name", bl.GROUPS_GRIDS)
def test_groups_model_equals_oracle_and_host_twin(ca, grid_name):
    for B in bl.GROUPS_B:
        p = bl.groups_problem(grid_name, B)
        assert p.row_ok.all()
        for g in range(p.G):
            rows = slice(g * B, (g + 1) * B)
            o_sh, o_ns = _oracle(p.grid, p.ages[g], p.weights[g], p.tabs[g])
            h_sh, h_ns = ca.bootstrap_counts_from_weights(p.grid, p.ages[g], p.weights[g], *p.tabs[g])
            assert np.array_equal(p.csh[rows], o_sh) and np.array_equal(p.cns[rows], o_ns), (grid_name, B, g)
            assert np.array_equal(p.csh[rows], h_sh) and np.array_equal(p.cns[rows], h_ns), (grid_name, B, g)


def _check_sums_exact(weights, tabs, reps, what):
    finite = [np.where(np.isfinite(t), t, 0.0) for t in tabs]  # (skipinf: block 0 is never summed; checked by its weight)
    for w, rep in zip(weights, reps):
        assert all(w[j] == 0 for j in range(len(w)) if not np.isfinite([t[j] for t in tabs]).all())
        for k in range(4):
            exact, bound = bl.exact_sum_bound(w, finite[k])
            err = np.abs(rep.sums[k] - exact)
            assert (err <= bound).all(), (what, k, float(err.max()), float(bound[np.argmax(err)]))


def test_model_sums_against_exact_arithmetic():
    """Each weighted block sum of the model lies within nb * 2**-53 * sum |w * t| of math.fsum of the exact products (the
    derived bound of a length-nb recursive sum, exact_sum_bound).  The sums do not depend on the grid kind, and on the age
    only through the zeroed part of emp_below, so one grid and the mid-grid age per (A, nb, tables) covers them; the
    groups problem adds nb = 115 and the product's own multinomial weights."""
    n = 0
    for A in bl.A_VALUES:
        for c in bl.matrix_cases(A):
            if c.grid_kind == "rand" and c.ai == 3:
                _check_sums_exact(c.weights, c.tabs, bl.matrix_model(A)[c.key][2], c)
                n += 1
    assert n == len(bl.A_VALUES) * len(bl.NB_VALUES) * len(bl.TABLE_KINDS)
    p = bl.groups_problem("ref185", 5)
    for g in range(p.G):
        _, _, reps = bl.model_counts(p.grid, p.ages[g], p.weights[g], p.tabs[g])
        _check_sums_exact(p.weights[g], p.tabs[g], reps, ("groups", g))


def test_cases_are_what_their_names_say():
    seen = {k: 0 for k in bl.TABLE_KINDS}
    for A in bl.A_VALUES:
        model = bl.matrix_model(A)
        for c in bl.matrix_cases(A):
            want = bl.intended_bin_start(A, c.grid_kind, c.ai)
            assert c.bin_start == want and c.outside == (want >= A), c
            if c.outside:
                continue
            csh, cns, reps = model[c.key]
            assert all(r.bin_start == want for r in reps), c
            assert reps[bl.ZERO_REPLICATE].normf == 0 and not csh[bl.ZERO_REPLICATE].any() and not cns[bl.ZERO_REPLICATE].any(), c
            assert (c.weights[2] == 1).all() or c.tables == "skipinf"
            live = [r for i, r in enumerate(reps) if c.weights[i].any()]
            seen[c.tables] += len(live)
            for r in live:
                if c.tables in ("noemp", "emp_below"):
                    assert r.normf == 0 and r.fcount == 0 and np.array_equal(r.csh, r.sums[0]), c  # 0/0 -> NaN -> 0
                    if c.tables == "emp_below" and want > 1 and c.nb == 9:
                        assert r.sums[2][:want].any(), c  # there ARE emp counts, all below bin_start
                if c.tables == "emp_last":
                    she, nse = r.sums[2][A - 1], r.sums[3][A - 1]
                    assert she > 0 and not r.sums[2][:A - 1].any(), c
                    assert r.F[A - 1] == she / (she + nse) > 0 and r.normf == r.F[A - 1], c  # unscaled, alone
                    assert r.csh[A - 1] == r.sums[0][A - 1] + r.F[A - 1] / r.normf * r.fcount, c
                if c.tables == "emp_shonly":
                    assert not r.sums[3].any(), c
                if c.tables == "dense" and c.nb == 9:
                    assert r.normf > 0 and (r.csh > r.sums[0]).any(), c  # something was redistributed
            if c.tables == "skipinf":
                assert not all(np.isfinite(t).all() for t in c.tabs) and (c.weights[:, 0] == 0).all(), c
                assert np.isfinite(csh).all() and np.isfinite(cns).all(), c
                if c.nb > 1:  # without the skip, block 0 would have reached these sums as 0 * inf and 0 * nan
                    assert c.weights[:bl.ZERO_REPLICATE].any(axis=1).all() and np.isinf(c.tabs[0][0]).any() and np.isnan(c.tabs[2][0, A - 1])
    assert all(v > 0 for v in seen.values()), seen


def test_outside_the_grid_is_an_error_of_the_host_twin(ca):
    for c in bl.outside_cases():
        assert bl.model_replicate(c.grid, c.age, c.weights[0], *c.tabs).outside, c
        with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
            ca.bootstrap_counts_from_weights(c.grid, c.age, c.weights, *c.tabs)
    p = bl.groups_problem("ref185", 3, outside=True)
    with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
        ca.bootstrap_counts_from_weights(p.grid, p.ages[bl.OUTSIDE_GROUP], p.weights[bl.OUTSIDE_GROUP], *p.tabs[bl.OUTSIDE_GROUP])
    with pytest.raises(ca.ColateError, match="bad sizes"):  # A < 2
        ca.bootstrap_counts_from_weights(np.array([0.0]), 0.0, np.ones((1, 2)), *(np.ones((2, 1)),) * 4)


def test_shard_bounds_restated(ca):
    from colate_amd import distributed
    from colate_amd._lib import lib

    for R in (6, 18, 30):
        for world in (2, 3, 4, 7, R):
            got = [bl.shard_bounds(R, world, r) for r in range(world)]
            assert got == [tuple(distributed.shard_bounds(R, world, r)) for r in range(world)]
            lo, hi = ctypes.c_int(), ctypes.c_int()
            for r in range(world):
                lib.colate_shard_bounds(R, world, r, ctypes.byref(lo), ctypes.byref(hi))
                assert (lo.value, hi.value) == got[r]
            assert got[0][0] == 0 and got[-1][1] == R and all(a[1] == b[0] for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("fault, code", [("null", -1), ("E_1100", -4), ("unsorted_epochs", -1), ("max_iter_0", -1),
                                         ("no_devices", -1)])
def test_sharded_bootstrap_entry_points_validate_before_the_device(ca, fault, code):
    """colate_bootstrap_em_batch_sharded / _groups_sharded refuse a NULL array, E above the compiled limit, unsorted epochs,
    max_iter = 0 and an empty device list with the codes of the other host-pointer EM entry points, before a device is
    asked for (a check after it would show as COLATE_ENODEVICE = -2 where there is none)."""
    from colate_amd._lib import lib

    A, B, nb, G = 185, 2, 3, 2
    E = 1100 if fault == "E_1100" else 23
    grid = np.ascontiguousarray(ol.age_grid())
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dev = (ctypes.c_int * 1)(0)
    lead = (0 if fault == "no_devices" else 1, dev)
    ep1 = np.linspace(0.0, 1e5, E) if E != 23 else ol.epochs_from_bins("3,7,0.2", 0.0, 28.0)[0]
    ep1 = ep1[::-1] if fault == "unsorted_epochs" else ep1
    first = None if fault == "null" else ptr(grid)
    max_iter = 0 if fault == "max_iter_0" else 10
    tabs = np.ones((G * nb, A))
    for name, rows, epoch_rows in (("colate_bootstrap_em_batch_sharded", B, 1), ("colate_bootstrap_em_batch_groups_sharded", G * B, G)):
        ep, init = np.ascontiguousarray(np.tile(ep1, (epoch_rows, 1))), np.full((epoch_rows, E), 5e-5)
        w = np.ones((rows, nb))
        rates, ll, iters, flags = np.zeros((rows, E)), np.zeros(rows), np.zeros(rows, np.int32), np.zeros(rows, np.int32)
        em = (ptr(ep), ptr(init), max_iter, 0, 1e-7, 5e-9, ptr(rates), ptr(iters), ptr(ll), ptr(flags), None, None)
        if epoch_rows == 1:
            args = (rows, nb, E, A, first, 0.0, ptr(w)) + (ptr(tabs),) * 4 + em
        else:
            gnb, gage = np.full(G, nb, np.int32), np.zeros(G)
            args = (G, B, E, A, first, ptr(gnb), ptr(gage), ptr(w)) + (ptr(tabs),) * 4 + em
        assert getattr(lib, name)(*lead, *args) == code, (name, lib.colate_last_error())
