"""GPU: every build of the EM kernel a batch size can select, at its edges (tests/em_builds_lib.py).

The kernel (csrc/em_kernel_impl.hpp) is compiled into more than a dozen instantiations and the library picks one from the batch
size, the epoch count and the device's CU count (csrc/em_build.hpp).  They differ in more than their schedule: barriers per
iteration, which wave keeps the verdict's history, which wave computes role B's epoch values, the one-slot last-rate test, the
split affine scan, the register caps; and from #CUs + 1 replicates on two workgroups share a CU.  Each case below runs the same
replicates through the automatic build of a small batch, the three forced variants, both ends of the batch range of the capped
build and the first batch of the throughput layout, asserts the name of the build each run took, and holds them to each other
byte for byte and to the oracle with the suite's tolerances.  The last test asserts that the cases together launched every
instantiation for up to 256 epochs that the dispatch table lists.

Cases run 40 to 60 iterations unless they are about the stop rule: the steady-state loops take over after the first, the
iterations 0, 1, 2, 4, 8, 16, 32 go through the peeled copy that refreshes the tail model.

FLOOR: per case, the share of (replicate, epoch) entries the checker must find pinned in the oracle itself
(oracle_lib.stable_mask) -- measured on the CPU from the oracle alone, minus 0.01, rounded down; the measured value beside it."""
import numpy as np
import pytest

import em_builds_lib as eb
import oracle_lib as ol

pytestmark = pytest.mark.gpu

FLOOR = {
    "one_epoch_per_lane[2]": 0.99,  # measured 1.0000
    "one_epoch_per_lane[16]": 0.99,  # measured 1.0000
    "one_epoch_per_lane[17]": 0.99,  # measured 1.0000
    "one_epoch_per_lane[32]": 0.99,  # measured 1.0000
    "one_epoch_per_lane[33]": 0.99,  # measured 1.0000
    "one_epoch_per_lane[64]": 0.99,  # measured 1.0000
    "two_epochs_per_lane[65]": 0.99,  # measured 1.0000
    "two_epochs_per_lane[128]": 0.99,  # measured 1.0000
    "four_epochs_per_lane[129]": 0.99,  # measured 1.0000
    "four_epochs_per_lane[256]": 0.99,  # measured 1.0000
    "age_grids[1-12]": 0.82,  # measured 0.8333
    "age_grids[1-40]": 0.94,  # measured 0.9500
    "age_grids[2-12]": 0.82,  # measured 0.8333
    "age_grids[2-40]": 0.94,  # measured 0.9500
    "age_grids[64-12]": 0.99,  # measured 1.0000
    "age_grids[64-40]": 0.99,  # measured 1.0000
    "age_grids[65-12]": 0.99,  # measured 1.0000
    "age_grids[65-40]": 0.99,  # measured 1.0000
    "age_grids[130-12]": 0.99,  # measured 1.0000
    "age_grids[130-40]": 0.99,  # measured 1.0000
    "age_grids[256-12]": 0.99,  # measured 1.0000
    "age_grids[256-40]": 0.99,  # measured 1.0000
    "one_bin_group": 0.90,  # measured 0.9130
    "without_shared_counts": 0.99,  # measured 1.0000
    "without_not_shared_counts": 0.87,  # measured 0.8841
    "starting_rates_of_zero[22]": 0.99,  # measured 1.0000
    "starting_rates_of_zero[21-22]": 0.99,  # measured 1.0000
    "starting_rates_of_zero[7]": 0.99,  # measured 1.0000
    "starting_rates_of_zero[7-8-9-10]": 0.99,  # measured 1.0000
    "q_underflows": 0.99,  # measured 1.0000
    "iteration_limits[1-1000]": 0.96,  # measured 0.9710
    "iteration_limits[2-1000]": 0.96,  # measured 0.9710
    "iteration_limits[3-1]": 0.96,  # measured 0.9710
    "iteration_limits[40-0]": 0.96,  # measured 0.9710
    "iteration_limits[40-39]": 0.96,  # measured 0.9710
    "iteration_limits[40-40]": 0.96,  # measured 0.9710
    "iteration_limits[41-40]": 0.96,  # measured 0.9710
    "per_row[23]": 0.96,  # measured 0.9783
    "per_row[40]": 0.99,  # measured 1.0000
    "stop_rule": 0.99,  # measured 1.0000 (the oracle's iterations: 1001 and 2211)
    "sparse[a]": 0.88,  # measured 0.8913
    "sparse[b]": 0.99,  # measured 1.0000
}


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    assert colate_amd.device_count() >= 1
    return colate_amd


def _tables(K, **kw):
    from colate_amd import workloads

    grid = ol.age_grid()
    csh, cns = workloads.bootstrap_tables(grid, K, nb=9, scale=1.0, **kw)
    return grid, csh, cns


def _epochs(n):
    if n == 2:
        return np.array([0.0, 1e3])
    if n == 23:
        return ol.epochs_from_bins("3,7,0.2")[0]
    return np.concatenate([[0.0], np.geomspace(30, 3e5, n - 2), [4e6]])


def _bin_groups(csh, cns):
    """Per replicate: the bin groups of 64 its live bins take once the kernel has compacted them to the range that has data."""
    live = (csh > 0) | (cns > 0)
    return [(int(np.flatnonzero(r)[-1]) - int(np.flatnonzero(r)[0])) // 64 + 1 for r in live]


def _run(ca, case, *args, **kw):
    return eb.through_every_build(ca, *args, floor=FLOOR.get(case), **kw)


@pytest.mark.parametrize("E", [2, 16, 17, 32, 33, 64])
def test_one_epoch_per_lane(ca, E):
    """The three row counts of the scans (16, 32, 64 epochs), both sides of each row boundary, the smallest epoch count and the
    last with one epoch per lane; default age grid, live bins in two groups (role B's epoch values come from wave 3)."""
    grid, csh, cns = _tables(3)
    assert _bin_groups(csh, cns) == [2, 2, 2]
    _run(ca, f"one_epoch_per_lane[{E}]", grid, csh, cns, _epochs(E), max_iter=40)


@pytest.mark.parametrize("E", [65, 128])
def test_two_epochs_per_lane(ca, E):
    """<0, 2, 4>: the epoch work of a role split over two waves -- with two workgroups on a CU at the end of its batch range --
    against the throughput layout's <0, 2, 4, true>."""
    grid, csh, cns = _tables(3)
    _run(ca, f"two_epochs_per_lane[{E}]", grid, csh, cns, _epochs(E), max_iter=40)


@pytest.mark.parametrize("E", [129, 256])
def test_four_epochs_per_lane(ca, E):
    """The throughput layout only: a small batch against a batch beyond twice the CU count."""
    grid, csh, cns = _tables(3)
    _run(ca, f"four_epochs_per_lane[{E}]", grid, csh, cns, _epochs(E), max_iter=40)


@pytest.mark.parametrize("E", [12, 40])
@pytest.mark.parametrize("A", [1, 2, 64, 65, 130, 256])
def test_age_grids(ca, A, E):
    """One to four bin groups per role in every build, padding lanes, the retiring of the waves without bins, and two ages
    exactly on an epoch start (they belong to the epoch that starts there)."""
    rng = np.random.default_rng(A)
    ep = _epochs(E)
    grid = np.sort(np.exp(rng.uniform(np.log(2.0), np.log(4e5), A)))
    if A >= 64:
        grid[5] = ep[3]
        grid[6] = ep[3]
        grid = np.sort(grid)
    csh = rng.uniform(0, 30, (3, A)) * ((rng.uniform(size=(3, A)) < 0.7) | (A < 64)) * (1 - np.exp(-grid / 9000.0))
    cns = rng.uniform(0, 60, (3, A)) * ((rng.uniform(size=(3, A)) < 0.7) | (A < 64))
    # (one or two bins are not thinned: a replicate left with counts of one kind only has a degenerate maximum -- every rate to
    # infinity or to the floor, log-likelihood to 0 -- where the oracle's own log-likelihood moves by up to 1.3e-9 under the
    # checker's libm noise, a hundred times the tolerance it is held to here)
    # the tied bins carry not-shared counts only: with a shared count at an age exactly on an epoch start the checker's libm
    # noise turns the reference's log(1 - exp(-0)) into NaN, and the oracle pins nothing (stable fraction 0 .. 0.33)
    csh[:, grid == ep[3]] = 0.0
    assert A < 64 or ((grid == ep[3]).sum() == 2 and (cns[:, grid == ep[3]] > 0).any())
    _run(ca, f"age_grids[{A}-{E}]", grid, csh, cns, ep, max_iter=60)


@pytest.mark.parametrize("A", [65, 256])
def test_shared_counts_on_an_epoch_start_are_the_same_in_every_build(ca, A):
    """What test_age_grids has to leave out: shared counts at the two ages tied to an epoch start.  The checker's libm noise turns
    the reference's log(1 - exp(-0)) into NaN there and pins no epoch of the oracle, so there is no parity statement to make; the
    builds are held to each other byte for byte, and to finite rates."""
    rng = np.random.default_rng(A)
    ep = _epochs(40)
    grid = np.sort(np.exp(rng.uniform(np.log(2.0), np.log(4e5), A)))
    grid[5] = ep[3]
    grid[6] = ep[3]
    grid = np.sort(grid)
    csh = rng.uniform(0, 30, (3, A)) * (rng.uniform(size=(3, A)) < 0.7) * (1 - np.exp(-grid / 9000.0))
    cns = rng.uniform(0, 60, (3, A)) * (rng.uniform(size=(3, A)) < 0.7)
    assert (csh[:, grid == ep[3]] > 0).any(axis=1).sum() >= 2
    r, it, ll, fl = eb.through_every_build(ca, grid, csh, cns, ep, parity=False, max_iter=60)
    assert np.isfinite(r).all() and np.isfinite(ll).all() and (ca.status_flags(fl) == ca.FLAG_MAXITER).all()


def test_one_bin_group(ca):
    """All live bins inside one group of 64: the waves of the second group retire, the leaders keep the verdict's history
    themselves (verdict_wave = 0) and role B's leader computes its epoch values itself."""
    grid, csh, cns = _tables(3)
    csh[:, 70:] = 0.0
    cns[:, 70:] = 0.0
    assert _bin_groups(csh, cns) == [1, 1, 1]
    _run(ca, "one_bin_group", grid, csh, cns, _epochs(23), max_iter=40)


def test_replicate_without_shared_counts(ca):
    """Role A's waves have no live bin in one replicate: their scalar live mask is 0."""
    grid, csh, cns = _tables(3)
    csh[0, :] = 0.0
    _run(ca, "without_shared_counts", grid, csh, cns, _epochs(23), max_iter=40)


def test_replicate_without_not_shared_counts(ca):
    """Role B's affine scan runs on s_e = 0 in every epoch: T stays 0 whatever the multipliers are."""
    grid, csh, cns = _tables(3)
    cns[0, :] = 0.0
    _run(ca, "without_not_shared_counts", grid, csh, cns, _epochs(23), max_iter=40)


@pytest.mark.parametrize("zero", [[22], [21, 22], [7], [7, 8, 9, 10]], ids=lambda z: "-".join(map(str, z)))
def test_starting_rates_of_zero(ca, zero):
    """A last rate of 0: the last epoch does not absorb and the loops compiled per kind of wave hand over to the general loop.
    A rate of 0 in the middle: the epoch's numerator is 0 and the M-step copies the previous epoch's rate."""
    grid, csh, cns = _tables(3)
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[zero] = 0.0
    first, _, _ = _run(ca, "starting_rates_of_zero[%s]" % "-".join(map(str, zero)), grid, csh, cns, ep, init=init, max_iter=40)
    assert np.isfinite(first[0]).all()


def test_rate_so_large_that_q_underflows(ca):
    """exp(-lambda_e dt_e) = 0 in one epoch: every window product that contains it is 0 from there on."""
    grid, csh, cns = _tables(3)
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[6] = 1.0e4 / (ep[7] - ep[6])
    assert np.exp(-init[6] * (ep[7] - ep[6])) == 0.0
    _run(ca, "q_underflows", grid, csh, cns, ep, init=init, max_iter=40)


@pytest.mark.parametrize("max_iter,min_iter", [(1, 1000), (2, 1000), (3, 1), (40, 0), (40, 39), (40, 40), (41, 40)])
def test_iteration_limits(ca, max_iter, min_iter):
    """Every hand-over between the loops (the iterations before min_iter, those from min_iter on, and for some waves all of
    them): no steady iteration at all, a stop rule that fires at once, a cap below / at / just above min_iter."""
    grid, csh, cns = _tables(3, seed=5)
    csh[1, 70:] = 0.0
    cns[1, 70:] = 0.0  # a replicate whose data fit one bin group
    _run(ca, f"iteration_limits[{max_iter}-{min_iter}]", grid, csh, cns, _epochs(23), max_iter=max_iter, min_iter=min_iter,
         rel_tol=1e-3 if min_iter < 10 else 1e-7)


@pytest.mark.parametrize("E", [23, 40])
def test_per_row_epochs_and_starting_rates(ca, E):
    """The batched all-pairs layout (epochs_stride, init_stride = E) outside the free build: two epoch grids alternating over
    the rows, one row's starting rates doubled; tiled with their rows."""
    grid, csh, cns = _tables(4)
    ep_a = _epochs(E)
    ep_b = ep_a.copy()
    ep_b[2:-1] *= 1.1
    eps = np.stack([ep_a, ep_b, ep_a, ep_b])
    init = np.full(eps.shape, 1.0 / 20000.0)
    init[3] *= 2.0
    _run(ca, f"per_row[{E}]", grid, csh, cns, eps, init=init, rows=True, max_iter=40)


def test_to_the_reference_stop_rule(ca):
    """Two replicates to the reference's stop rule, of which one stops later than the other: the loops of the log-likelihood
    phase, and replicates of one launch ending in different iterations."""
    grid, csh, cns = _tables(3)
    csh, cns = csh[:2].copy(), cns[:2].copy()
    csh[1, 120:] = 0.0  # (the second replicate's old shared counts removed: it converges later)
    first, (r0, it0, ll0, fl0), mask = _run(ca, "stop_rule", grid, csh, cns, _epochs(23))
    assert it0[0] != it0[1] and (it0 >= 1001).all() and (fl0 == 0).all(), it0


def test_sparse_tables(ca):
    """The seven low-coverage-like replicates of test_sparse_tables_and_the_integ_residue (test_gpu_parity.py): the tail model's
    refresh and the deep floor in every build -- resolved epochs at the floor right behind a rate above 1e-3 where the reference
    has them."""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep = _epochs(23)
    csh, cns = workloads.sparse_tables(grid, 512)
    behind_spike = 0
    for part, idx in (("a", [97, 178, 246, 286]), ("b", [352, 3, 400])):  # the first five have epochs behind a rate spike
        first, (r0, it0, ll0, fl0), mask = _run(ca, f"sparse[{part}]", grid, csh[idx], cns[idx], ep)
        assert it0.max() > 1001
        for b in range(len(idx)):
            f = (r0[b, 1:] == 5e-9) & mask[b, 1:] & (np.maximum.accumulate(r0[b, :-1]) > 1e-3)
            behind_spike += bool(f.any())
            assert (first[0][b, 1:][f] == 5e-9).all()
        # (and the kernel's own verdict is safe: every epoch it calls resolved is within the tolerance)
        ol.check_rates(first[0], first[3], r0, mask, eb.RATE_RTOL)
    assert behind_spike >= 3  # the regime is really there


def test_every_build_up_to_256_epochs_was_reached(ca):
    """The cases above (this test runs after them) launched every instantiation the dispatch table lists for the EM fit at up to
    256 epochs: a new one cannot be added without a case that runs it.  The builds for more epochs are test_more_than_256_epochs'
    (test_gpu_parity.py)."""
    listed = {n for n in ca.em_kernel_builds(0) if not n.startswith("big-")}
    # (the set is filled by the cases of this file in this process: selected alone, with -k, --lf or in another worker, this
    # test has nothing to judge)
    assert eb.CASES_RUN >= len(FLOOR), (f"only {eb.CASES_RUN} of the {len(FLOOR)} cases of this file ran in this process before this "
                                        "test: run the whole file, in order, in one process")
    assert eb.REACHED - listed == set(), ("launched but not listed", sorted(eb.REACHED - listed))
    assert listed - eb.REACHED == set(), ("listed but launched by no case of this file", sorted(listed - eb.REACHED))
