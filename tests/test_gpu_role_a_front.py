"""GPU: role A's side of the two-barrier EM iteration (em_kernel_impl.hpp, em_role_a_front / kFront).

The build for batches that leave every workgroup a CU to itself issues role A's two chains in front of barrier 2 -- the cs scan
with exp(-cs_e), and the rate-only head of the bin terms -- interleaved by hand; the rate of a bin's epoch and the scan's first
operand are taken at the end of the iteration before.  Same operations on the same operands: each case runs `em_batch` through every build (latency-ilp, latency, throughput) and asserts that rates,
iteration counts, log-likelihood and flags are byte-equal across them, and that the rates are within the suite's tolerance of
the oracle wherever the checker finds the oracle itself stable (oracle_lib.stable_mask), with equal iteration counts.

Shapes: three replicates, the default age grid (185 bins), 40 iterations -- the steady-state loops run 39 of them."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
RATE_RTOL = 1e-6  # north_star: the tolerance of every oracle comparison of the suite
VARIANTS = ("latency-ilp", "latency", "throughput")
MAX_ITER = 40


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


def _epoch_of_bin(grid, ep):
    """The kernel's s_kb: the largest e with ep[e] <= age."""
    return np.maximum(np.searchsorted(ep, grid, side="right") - 1, 0)


def _bits(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def _check(ca, grid, csh, cns, ep, init=None, capped_build=False):
    """Runs every build, asserts byte-equality across them and parity with the oracle on its stable epochs; returns the outputs
    of the automatic build and the oracle's."""
    kw = dict(max_iter=MAX_ITER)
    okw = dict(kw) if init is None else dict(kw, init=init)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep, **okw)
    assert not (fl0 & 3).any(), "the reference aborts on this input: not a case"
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
    assert (it == it0).all(), (it, it0)
    mask = ol.stable_mask(grid, csh, cns, ep, r0, **okw)
    rel = np.abs(r - r0) / np.maximum(np.abs(r0), 1e-300)
    print(f"E={ep.size}: stable fraction {mask.mean():.3f}, max rel diff on it {rel[mask].max(initial=0.0):.3e}")
    assert rel[mask].max(initial=0.0) < RATE_RTOL, (float(rel[mask].max(initial=0.0)), mask.mean())
    return out["latency-ilp"], (r0, it0, ll0, fl0), mask


@pytest.mark.parametrize("E", [16, 17, 23, 31, 32, 33])
def test_two_bin_groups_around_the_epoch_rows(ca, tables, E):
    """Both sides of every boundary between one, two and four 16-lane rows of epochs (the scan in the front has one cross-row step
    more on the far side of each); live bins on both sides of lane 63 / 64 of the compacted tile: waves 0 and 2 both run the
    front.  23 epochs: also tiled to 258 rows, through the capped build."""
    grid, csh, cns = tables
    assert all(last - first + 1 > 64 for first, last in _live_span(csh, cns))
    _check(ca, grid, csh, cns, _epochs(E), capped_build=(E == 23))


@pytest.mark.parametrize("E", [16, 23, 32])
def test_one_bin_group(ca, tables, E):
    """All live bins inside one group of 64: waves 2 and 3 retire and wave 0 runs the loop of the leader that also keeps the
    verdict's history."""
    grid, csh, cns = tables
    csh, cns = csh.copy(), cns.copy()
    csh[:, 70:] = 0.0
    cns[:, 70:] = 0.0
    assert all(last - first + 1 <= 64 for first, last in _live_span(csh, cns))
    _check(ca, grid, csh, cns, _epochs(E))


def test_replicate_without_shared_counts(ca, tables):
    """Role A's waves of replicate 0 have no bin with data: the scalar mask of the lanes with data is 0, every product of the bin
    terms a zero, the suffix sum runs on zeros."""
    grid, csh, cns = tables
    csh = csh.copy()
    csh[0, :] = 0.0
    _check(ca, grid, csh, cns, _epochs(23))


def test_epoch_without_bins_and_epoch_across_a_row(ca, tables):
    """An epoch that holds no age bin (no lane fetches its rate or its S_e) and an epoch whose bins lie on both sides of a 16-lane
    row boundary of the compacted tile (two tail slots)."""
    grid, csh, cns = tables
    ep = _epochs(23).copy()
    # epochs 10 and 11 start between two neighbouring ages of the grid: epoch 10 is empty
    j = int(np.searchsorted(grid, ep[10], side="right")) - 1
    assert ep[9] <= grid[j] and grid[j + 1] < ep[12]
    ep[10] = grid[j] + 0.3 * (grid[j + 1] - grid[j])
    ep[11] = grid[j] + 0.6 * (grid[j + 1] - grid[j])
    assert (np.diff(ep[1:]) > 0).all()  # (the first two epochs of this grid both start at 0)
    kb = _epoch_of_bin(grid, ep)
    assert not (kb == 10).any() and (kb == 9).any() and (kb == 11).any()
    straddles = 0
    for first, last in _live_span(csh, cns):
        pos = np.arange(first, last + 1) - first  # position in the compacted tile
        k = kb[first:last + 1]
        for e in np.unique(k):
            rows = np.unique(pos[k == e] >> 4)
            assert rows.size <= 2, "more than two tail slots: the general loop, not a case"
            straddles += int(rows.size == 2)
    assert straddles > 0
    _check(ca, grid, csh, cns, ep)


@pytest.mark.parametrize("zero", [[7], [7, 8, 9, 10]])
def test_epoch_whose_numerator_becomes_zero(ca, tables, zero):
    """A rate of 0 in the middle: the bin's 1 / lambda_k is taken in every lane and selected to 0, the epoch's numerator is 0 and
    the M-step's copy path -- out of line -- leaves and re-enters the loop with the fetched rate and the scan's first operand."""
    grid, csh, cns = tables
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[zero] = 0.0
    (r, it, ll, fl), _, _ = _check(ca, grid, csh, cns, ep, init=init)
    assert np.isfinite(r).all()


def test_last_rate_of_zero(ca, tables):
    """The last epoch does not absorb: the steady-state loops are left at once, barrier 1 is executed, and the general loop runs
    the parent's code."""
    grid, csh, cns = tables
    ep = _epochs(23)
    init = np.full(ep.size, 1.0 / 20000.0)
    init[22] = 0.0
    _check(ca, grid, csh, cns, ep, init=init)


def test_shared_bin_in_the_last_epoch(ca, tables):
    """Shared counts in bins beyond the start of the last epoch: t_{k+1} does not exist there (end of epoch 0, length 0)."""
    grid, csh, cns = tables
    ep = _epochs(23).copy()
    first, last = max(f for f, _ in _live_span(csh, cns)), min(l for _, l in _live_span(csh, cns))
    # all epoch starts scaled down so that the last epoch starts three bins below the oldest bin that carries data in every replicate
    ep *= 0.5 * (grid[last - 3] + grid[last - 2]) / ep[22]
    kb = _epoch_of_bin(grid, ep)
    csh = csh.copy()
    csh[:, last - 1] = np.maximum(csh[:, last - 1], 2.0)
    assert (kb[last - 1] == 22) and (csh[:, kb == 22] > 0).any(axis=1).all() and first < last - 3
    _check(ca, grid, csh, cns, ep)
