"""GPU: role B's affine scan in two parts (em_kernel_impl.hpp, em_affine_split / kHoist).

The build for batches that leave every workgroup a CU to itself computes the multipliers of the scan T_{e+1} = q_e T_e + s_e
-- window products of the q_e -- in front of barrier 2 and runs the data half alone behind it; every other build keeps the
single scan.  Same operations on the same operands: each case runs `em_batch` through every build and asserts that rates,
iteration counts, log-likelihood and flags are bit-identical across them, and that the rates are within the parity tolerance
of the oracle wherever the checker finds the oracle itself stable (oracle_lib.stable_mask).

Shapes: three replicates, the default age grid (185 bins), 40 iterations unless a case says otherwise -- the steady-state
loops run 39 of them, the iterations 0, 1, 2, 4, 8, 16, 32 through the peeled copy that refreshes the tail model."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
RATE_RTOL = 1e-6  # north_star: the tolerance of every oracle comparison of the suite
VARIANTS = ("latency-ilp", "latency", "throughput")


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    assert colate_amd.device_count() >= 1
    return colate_amd


@pytest.fixture(scope="module")
def tables():
    """(grid, shared counts, not-shared counts) of three replicates; read-only for the tests (they copy before they edit)."""
    from colate_amd import workloads

    grid = ol.age_grid()
    csh, cns = workloads.bootstrap_tables(grid, 3, nb=9, scale=1.0)
    csh.setflags(write=False)
    cns.setflags(write=False)
    return grid, csh, cns


def _epochs(n):
    if n == 23:
        return ol.epochs_from_bins("3,7,0.2")[0]
    return np.concatenate([[0.0], np.geomspace(30, 3e5, n - 2), [4e6]])


def _live_span(csh, cns):
    """Per replicate: (first, last) bin with data of either kind -- the kernel compacts the bins to that range, 64 per wave."""
    live = (csh > 0) | (cns > 0)
    return [(int(np.flatnonzero(r)[0]), int(np.flatnonzero(r)[-1])) for r in live]


def _bits(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def _check(ca, grid, csh, cns, ep, init=None, max_iter=40, capped_build=False):
    """Runs every build, asserts bit-identity across them and parity with the oracle on its stable epochs; returns the
    outputs of the automatic build and the oracle's."""
    kw = dict(max_iter=max_iter)
    out = {}
    for variant in VARIANTS:
        ca.em_force_variant(variant)
        try:
            assert ca.em_kernel_variant(csh.shape[0], ep.size) == variant
            out[variant] = ca.em_batch(grid, csh, cns, ep, init_rates=init, **kw)
        finally:
            ca.em_force_variant(None)
    if capped_build:
        # beyond the CU count (256) two workgroups share a CU and the max-ilp unit runs its build with the register cap and three
        # barriers per iteration: the same replicates, tiled to a batch of 258, through that build
        reps = 86
        big = ca.em_batch(grid, np.tile(csh, (reps, 1)), np.tile(cns, (reps, 1)), ep, init_rates=init, **kw)
        out["latency-ilp, capped"] = tuple(a[:csh.shape[0]] for a in big)
        for a in big:  # (and every copy of a replicate agrees with the first)
            assert _bits([a[:csh.shape[0]]] * reps) == _bits([a[k * csh.shape[0]:(k + 1) * csh.shape[0]] for k in range(reps)])
    names = ("rates", "iterations", "loglik", "flags")
    for other in out:
        for name, a, b in zip(names, _bits(out["latency-ilp"]), _bits(out[other])):
            assert a == b, (other, name)
    r, it, ll, fl = out["latency-ilp"]
    okw = dict(kw) if init is None else dict(kw, init=init)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep, **okw)
    assert not (fl0 & 3).any(), "the reference aborts on this input: not a case"
    assert (it == it0).all(), (it, it0)
    mask = ol.stable_mask(grid, csh, cns, ep, r0, **okw)
    rel = np.abs(r - r0) / np.maximum(np.abs(r0), 1e-300)
    print(f"E={ep.size} max_iter={max_iter}: stable fraction {mask.mean():.3f}, max rel diff on it {rel[mask].max(initial=0.0):.3e}")
    assert rel[mask].max(initial=0.0) < RATE_RTOL, (float(rel[mask].max(initial=0.0)), mask.mean())
    return out["latency-ilp"], (r0, it0, ll0, fl0), mask


@pytest.mark.parametrize("E", [16, 17, 23, 32, 33])
def test_epoch_counts_around_the_scan_rows(ca, tables, E):
    """One, two and four 16-lane rows of epochs and both sides of the row boundaries, where the scan's cross-row steps
    (row_bcast15, row_bcast31) start to matter; the live bins lie on both sides of lane 63 / 64 of the compacted tile (two bin
    groups: role B's epoch values come from wave 3 and the leader takes q_e from its own rates)."""
    grid, csh, cns = tables
    assert all(last - first + 1 > 64 for first, last in _live_span(csh, cns))
    _check(ca, grid, csh, cns, _epochs(E), capped_build=(E == 23))


def test_split_kernel_at_65_epochs(ca, tables):
    """Two epochs per lane, the epoch work of a role split over two waves: an owner takes the other slot's q_e from LDS."""
    grid, csh, cns = tables
    _check(ca, grid, csh, cns, _epochs(65))


def test_one_bin_group(ca, tables):
    """All live bins inside one group of 64: waves 2 and 3 retire, role B's leader computes q_e, p_e, beta_e itself."""
    grid, csh, cns = tables
    csh, cns = csh.copy(), cns.copy()
    csh[:, 70:] = 0.0
    cns[:, 70:] = 0.0
    assert all(last - first + 1 <= 64 for first, last in _live_span(csh, cns))
    _check(ca, grid, csh, cns, _epochs(23))


def test_replicate_without_not_shared_counts(ca, tables):
    """The scan runs on s_e = 0 in every epoch: T stays 0 whatever the multipliers are."""
    grid, csh, cns = tables
    cns = cns.copy()
    cns[0, :] = 0.0
    _check(ca, grid, csh, cns, _epochs(23))


@pytest.mark.parametrize("zero", [[22], [21, 22]])
def test_last_rate_of_zero(ca, tables, zero):
    """The last epoch does not absorb: the loops compiled per kind of wave hand over to the general loop, which keeps the
    single scan in every build."""
    grid, csh, cns = tables
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[zero] = 0.0
    _check(ca, grid, csh, cns, ep, init=init)


@pytest.mark.parametrize("zero", [[7], [7, 8, 9, 10]])
def test_epoch_with_a_numerator_of_zero(ca, tables, zero):
    """A rate of 0 in the middle: nothing coalesces in the epoch, its numerator is 0 and the M-step copies the previous epoch's
    rate -- a rate repeated across epochs, and the copy path of the M-step in front of the hoisted products."""
    grid, csh, cns = tables
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[zero] = 0.0
    (r, it, ll, fl), _, _ = _check(ca, grid, csh, cns, ep, init=init)
    assert np.isfinite(r).all()


def test_rate_so_large_that_q_underflows(ca, tables):
    """exp(-lambda_e dt_e) = 0 in one epoch: every window product that contains it is 0 from there on."""
    grid, csh, cns = tables
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[6] = 1.0e4 / (ep[7] - ep[6])  # lambda dt = 1e4: exp(-1e4) underflows to 0
    assert np.exp(-init[6] * (ep[7] - ep[6])) == 0.0
    _check(ca, grid, csh, cns, ep, init=init)


def test_to_the_reference_stop_rule(ca, tables):
    """Two replicates to the reference's stop rule (1001 iterations at the earliest): every refresh iteration of the tail model
    -- which reads q_e T_e -- and the hand-over to the loops of the log-likelihood phase."""
    grid, csh, cns = tables
    (r, it, ll, fl), (r0, it0, ll0, fl0), mask = _check(ca, grid, csh[:2], cns[:2], _epochs(23), max_iter=100000)
    assert (it >= 1001).all() and (ca.status_flags(fl) == 0).all()
    assert np.allclose(ll, ll0, rtol=1e-11, atol=0)
