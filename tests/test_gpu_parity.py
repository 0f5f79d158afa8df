"""GPU parity: the HIP path (through the C ABI) against the oracle on the same inputs.

Tolerances (north_star): rates within 1e-6 relative; here the E-step statistics and the
rates are held to much tighter bounds wherever the reference's own arithmetic is
well-conditioned (see oracle_lib.stable_mask and DESIGN.md §6 for the one exception)."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

RATE_RTOL = 1e-6  # north_star tolerance on rates


def _rel(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    m[m == 0] = 1.0
    return np.abs(a - b) / m


def _den_tol(D0, ep, total_count):
    """Tolerance for E-step denominators: 1e-6 relative, plus the rounding residue the reference
    itself carries: its `integ = 1 - num[0] - num[1] - ...` (coal_EM.cpp:270-274, 445-449) sums
    terms exp(A - Z) whose relative error is ~1e-16*|A - Z| (hundreds at high rates), so integ is
    exact only to ~1e-14 absolute, and it enters denom[e] multiplied by the epoch length
    (DESIGN.md §6).  1e-13 * dt is that residue's scale, not a slack on real signal."""
    dt = np.append(np.diff(ep), 0.0)
    return 1e-6 * np.abs(D0) + 1e-13 * dt * total_count + 1e-300


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    assert colate_amd.device_count() >= 1
    return colate_amd


@pytest.mark.parametrize("bins", ["3,7,0.2", "2,7.95,0.05"])
def test_estep_matches_oracle(ca, bins):
    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins(bins)
    E, A = ep.size, grid.size
    rng = np.random.default_rng(7)
    B = 24
    rates = np.zeros((B, E))
    csh = np.zeros((B, A))
    cns = np.zeros((B, A))
    for t in range(B):
        if t < 5:
            rates[t] = 1e-6 * 10 ** t
        else:
            rates[t] = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), E))
            if t % 3 == 0:
                rates[t, : rng.integers(1, 4)] = 0.0
            if t % 4 == 0:
                rates[t, rng.integers(0, E, 3)] = 5e-9
        csh[t] = np.where(rng.uniform(size=A) < 0.8, rng.uniform(0, 50, A), 0.0)
        cns[t] = np.where(rng.uniform(size=A) < 0.8, rng.uniform(0, 500, A), 0.0)
        if t % 2:
            csh[t, :40] = cns[t, :40] = 0
            csh[t, 151:] = cns[t, 151:] = 0
    num, den, ll, flags = ca.em_estep(grid, csh, cns, ep, rates)
    checked = 0
    for t in range(B):
        N0, D0, ll0, fl0 = ol.estep(ep, rates[t], grid, csh[t], cns[t])
        if fl0:  # the reference aborts on this input (assert !isnan, coal.cpp:3711): nothing to compare
            continue
        checked += 1
        assert flags[t] == 0
        assert abs(ll[t] - ll0) <= 1e-12 * abs(ll0)
        assert _rel(num[t], N0).max() < 1e-8
        assert (np.abs(den[t] - D0) <= _den_tol(D0, ep, csh[t].sum() + cns[t].sum())).all()
    assert checked >= B - 2


def test_em_matches_oracle_wholegenome_like(ca):
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    csh, cns = workloads.bootstrap_tables(grid, 6)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert (fl0 == 0).all() and (fl1 == 0).all()  # flags 0: clean AND no epoch below the reference's resolution
    assert (it0 == it1).all()
    assert np.allclose(ll1, ll0, rtol=1e-12, atol=0)
    assert _rel(r1, r0).max() < RATE_RTOL
    assert _rel(r1, r0).max() < 1e-9  # what we actually get
    assert ol.stable_mask(grid, csh, cns, ep, r0).all()  # the checker agrees: all 23 epochs are pinned


def test_em_matches_oracle_122_epochs(ca):
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins("2,7.95,0.05")
    csh, cns = workloads.bootstrap_tables(grid, 3, nb=9, scale=1.0)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert (it0 == it1).all() and (ca.status_flags(fl1) == 0).all()
    assert np.allclose(ll1, ll0, rtol=1e-12, atol=0)
    noise, scaled = ol.rerun_rates(grid, csh, cns, ep)
    mask = ol.mask_from_reruns(r0, noise + scaled)
    unres, unstable = ol.check_rates(r1, fl1, r0, mask, RATE_RTOL)
    # only the far tail is undetermined in the reference: 104+ of 122 epochs are pinned (measured: 105-106), and the
    # kernel flags that tail itself: the checker's count +- 1 (its own count moves by one between noise seeds), at most 2 more
    assert (unstable <= 18).all() and (unres >= unstable - 1).all() and (unres <= unstable + 2).all(), (unres, unstable)
    # ... and inside that tail the kernel stays within the reference's own noise envelope wherever the reference is
    # reproducible at all: the kernel models what IEEE arithmetic makes of the reference's `integ` recurrence (absorbed
    # log-sum-exp terms, the clamp, rounding noise).  Measured over 32 whole-genome replicates
    # (profiles/parity/): median ratio ~1, 90th percentile 2.3, maximum 5.5 with the spread estimated from three reruns.
    ratio, spread = ol.noise_envelope(r1, r0, noise)
    zone = (spread > 1e-9) & (spread < 0.05)
    assert zone.sum() >= 9 and np.median(ratio[zone]) <= 3.0 and ratio[zone].max() <= 12.0, (np.median(ratio[zone]), ratio[zone].max())


@pytest.mark.parametrize("bins,E_expect", [("3,7,0.3", 17), ("3,7,0.1", 43), ("3,7,0.07", 61), ("2,7.95,0.03", 202),
                                           ("2,7.9,0.024", 249)])
def test_every_kernel_instantiation(ca, bins, E_expect):
    """The EM kernel is instantiated per epoch-count range (1, 2 or 4 rows of 16 epochs in one chunk of 64;
    2 and 4 chunks up to 256 epochs): a short EM (same iteration cap on both sides) and one E-step for an epoch
    count in each range; 17 / 23 / 122 epochs are covered by the other tests."""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins(bins)
    assert ep.size == E_expect
    csh, cns = workloads.bootstrap_tables(grid, 2, nb=9, scale=1.0)
    kw = dict(max_iter=60, min_iter=20)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep, **kw)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep, **kw)
    assert (it0 == it1).all() and ((fl0 & 3) == 0).all() and (fl0 == ca.status_flags(fl1)).all()
    assert np.allclose(ll1, ll0, rtol=1e-12, atol=0)
    mask = ol.stable_mask(grid, csh, cns, ep, r0, **kw)
    # (the checker's own stable fraction, measured: 1.0 up to 64 epochs, 0.86 / 0.87 at 202 / 249 epochs)
    assert mask.mean() > (0.99 if ep.size <= 64 else 0.85), mask.mean()
    assert _rel(r1, r0)[mask].max() < RATE_RTOL
    # one E-step at the rates the EM arrived at
    num, den, ll, flags = ca.em_estep(grid, csh, cns, ep, r0)
    for t in range(2):
        N0, D0, l0, f0 = ol.estep(ep, r0[t], grid, csh[t], cns[t])
        assert f0 == 0 and flags[t] == 0
        assert abs(ll[t] - l0) <= 1e-12 * abs(l0)
        assert _rel(num[t], N0).max() < 1e-8
        assert (np.abs(den[t] - D0) <= _den_tol(D0, ep, csh[t].sum() + cns[t].sum())).all()


def test_sparse_tables_and_the_integ_residue(ca):
    """Low-coverage-like tables (a few mutations per age bin): irregular convergence, single epochs with very
    high rates, and behind them epochs whose survival probability is below the resolution of the reference's
    `integ = 1 - num[0] - ...`: there the reference's denominator is the rounding residue of that subtraction and
    its rate drops to the floor.  The kernel models what that residue is made of -- for the not-shared kind the expectation
    s_b H((x_be - D_b) / s_b) of the frozen rounding error per (bin, epoch), for the shared kind a mean per unit count in the
    epochs a bin's chain reaches (em_kernel_impl.hpp, `tail model`) --: same iteration counts, rates within
    1e-6 on every resolved epoch, the floor where the reference has it."""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    csh, cns = workloads.sparse_tables(grid, 512)
    idx = [97, 178, 246, 286, 352, 3, 400]  # the first five have epochs behind a rate spike (cumsum > 45)
    csh, cns = csh[idx], cns[idx]
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert ((fl0 & 3) == 0).all() and (ca.status_flags(fl1) == fl0).all()
    assert (it0 == it1).all() and it0.max() > 1001
    assert np.allclose(ll1, ll0, rtol=1e-11, atol=0)
    mask = ol.stable_mask(grid, csh, cns, ep, r0)
    assert mask.mean() > 0.93, mask.mean()  # (measured: 0.938)
    ol.check_rates(r1, fl1, r0, mask, RATE_RTOL)
    # the regime is really there: resolved epochs at the floor right behind a rate above 1e-3, in several replicates
    floor_behind_spike = [(r0[b, 1:] == 5e-9) & mask[b, 1:] & (np.maximum.accumulate(r0[b, :-1]) > 1e-3) for b in range(len(idx))]
    assert sum(f.any() for f in floor_behind_spike) >= 3
    for b, f in enumerate(floor_behind_spike):
        assert (r1[b, 1:][f] == 5e-9).all()


def test_underflow_snapshot_epoch_is_flagged(ca):
    """A replicate whose last epoch's numerator underflows to exactly 0 for a few hundred iterations ("num == 0: copy the
    previous rate", coal.cpp:3779-3788) and recovers: the rate freezes at whatever its neighbour was at that moment --
    the oracle's own value moves by tens of per cent under 1-ulp libm noise.  The kernel must not call it resolved."""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    csh, cns = workloads.sparse_tables(grid, 192)
    csh, cns = csh[82:83], cns[82:83]
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert (it0 == it1).all() and (ca.status_flags(fl1) == 0).all()
    mask = ol.stable_mask(grid, csh, cns, ep, r0)
    assert not mask[0, -1]  # the checker sees it
    unres, unstable = ol.check_rates(r1, fl1, r0, mask, RATE_RTOL)
    assert unres[0] >= 1  # ... and so does the kernel


def test_coal_EM_mirror_reference_unit_test(ca):
    """Restates TEST_CASE("test EM expectation step") (include/test/test_aDNA.cpp:68-212) with the
    GPU class in place of coal_EM and the oracle in place of coal_EM_simplified, at 1e-9 instead of
    the reference test's 10 %."""
    E = 21
    ypg = np.float32(28.0)
    ep = np.zeros(E)
    ep[1] = 1e3 / 28.0
    log10 = float(np.float32(np.log(10)))
    for e in range(2, E - 1):
        ep[e] = np.exp(log10 * (3.0 + 4.0 * (e - 1.0) / (E - 3.0))) / 28.0
    ep[E - 1] = 1e8 / 28.0
    C = 5
    nb = int(np.log(1e8) * C)
    ages = np.exp(np.arange(nb) / C) / 10.0
    for f in range(1, 8):
        rate = 1e-7 * np.exp(np.log(10) * (f - 1))
        rates = np.full(E, rate)
        em = ca.coal_EM(ep, rates)
        for kind, shared in ((0, True), (1, False)):
            num, den, ll, flags = em.EM_many(ages, shared)
            for b, a in enumerate(ages):
                l0, n0, d0 = ol.em_call(kind, ep, rates, a)
                assert abs(ll[b] - l0) < 1e-9 * max(1.0, abs(l0))
                assert np.all(num[b] >= 0) and np.all(den[b] >= 0)
                assert _rel(num[b], n0).max() < 1e-7
                assert (np.abs(den[b] - d0) <= _den_tol(d0, ep, 1.0)).all()


@pytest.mark.parametrize("bins,E_expect", [("3,7,0.01", 404), ("2,7.95,0.01", 598), ("2,7.99,0.006", 1002)])
def test_more_than_256_epochs(ca, bins, E_expect):
    """The reference builds and runs any number of epochs (coal.cpp:3551-3632: `--bins 3,7,0.01` gives 404); so does the drop-in,
    up to 1024, on the 8- and 16-epochs-per-lane instantiations (csrc/em_kernels_big.hip): full EM runs to the reference's stop
    rule against the oracle -- iteration counts, log-likelihood, every rate the checker finds pinned -- and one E-step."""
    from colate_amd import workloads

    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins(bins)
    assert ep.size == E_expect
    csh, cns = workloads.bootstrap_tables(grid, 2, nb=9, scale=1.0)
    r0, it0, ll0, fl0 = ol.em_batch(grid, csh, cns, ep)
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert (it0 == it1).all() and ((fl0 & 3) == 0).all() and (ca.status_flags(fl1) == 0).all()
    assert np.allclose(ll1, ll0, rtol=1e-12, atol=0)
    # the same two replicates tiled to the first batch beyond twice the CU count (asked from the library, as in
    # tests/em_builds_lib.py): the same instantiation with several workgroups on a CU, every row byte for byte the small batch's
    B = next(b for b in range(1, 4096) if ca.em_kernel_variant(b, 64) == "throughput")
    assert ca.em_kernel_build(2, ep.size) == ca.em_kernel_build(B, ep.size) == ("big-tput/8x4" if ep.size <= 512 else "big-tput/16x4")
    idx = np.arange(B) % 2
    for a, b in zip((r1, it1, ll1, fl1), ca.em_batch(grid, csh[idx], cns[idx], ep)):
        assert b.shape[0] == B and np.ascontiguousarray(a[idx]).tobytes() == b.tobytes()
    noise, scaled = ol.rerun_rates(grid, csh, cns, ep)
    mask = ol.mask_from_reruns(r0, noise + scaled)
    assert mask.mean() > 0.8, mask.mean()
    ol.check_rates(r1, fl1, r0, mask, RATE_RTOL)
    rates = np.exp(np.random.default_rng(E_expect).uniform(np.log(2e-6), np.log(3e-4), (2, ep.size)))
    N1, D1, l1, f1 = ca.em_estep(grid, csh, cns, ep, rates)
    for b in range(2):
        N0, D0, l0, f0 = ol.estep(ep, rates[b], grid, csh[b], cns[b])
        ok = D0 > 1e-250
        assert f0 == 0 and f1[b] == 0 and abs(l1[b] / l0 - 1) < 1e-12
        # (numerators to rounding; denominators to 1e-7 where they are more than the reference's integ residue, dt_e x ~1e-16 per
        # unit count, which the kernel models -- DESIGN.md section 6 -- instead of reproducing bit for bit)
        okd = ok & (D0 > 1e-6 * D0.max())
        assert _rel(N1[b][ok], N0[ok]).max() < 1e-9 and _rel(D1[b][okd], D0[okd]).max() < 1e-7 and okd.sum() > 0.8 * ep.size


def test_tail_at_122_epochs_lies_inside_the_range_of_the_references_real_builds(ca):
    """Where the reference stops reproducing ITSELF (tools/ref_self_reproducibility.py: six real builds of its unmodified sources
    print identical tokens up to epoch 105 of 122 and differ by 15 % at epoch 109, by orders of magnitude beyond) the kernel must
    print what those builds could print: token-identical to the stock build up to epoch 105, within three of the builds' own
    spreads at 107 and 108, and at 109 -- the epoch in which the rate falls from 5e-5 towards the floor; round 3 printed 6e-6
    there, outside every build -- inside the range the builds span over the 64 replicates, as at 110 and 111."""
    from colate_amd import workloads

    fix, f0, built, it_stock = ol.observed_spread_e122()
    t = fix["table"]
    grid = ol.age_grid()
    ep, _ = ol.epochs_from_bins(fix["bins"])
    csh, cns = workloads.bootstrap_tables(grid, t["replicates"], nb=t["nb"], scale=t["scale"], ne2=t["ne2"], seed=t["seed"])
    r1, it1, ll1, fl1 = ca.em_batch(grid, csh, cns, ep)
    assert it1.tolist() == it_stock and (ca.status_flags(fl1) == 0).all()
    gpu = np.array([[float("%g" % x) for x in row[f0:]] for row in r1])  # as printed, like the builds
    stock, others = built["base"], [v for k, v in built.items() if k != "base"]
    lo = np.minimum.reduce([stock] + others)
    hi = np.maximum.reduce([stock] + others)
    spread = np.max([np.abs(o - stock) for o in others], axis=0) / stock
    for e in range(f0, 106):  # every build prints the same token: so does the kernel
        assert (gpu[:, e - f0] == stock[:, e - f0]).all(), e
    for e in (107, 108):
        rel = np.abs(gpu[:, e - f0] - stock[:, e - f0]) / stock[:, e - f0]
        assert np.median(rel) <= 3.0 * np.median(spread[:, e - f0]), (e, np.median(rel), np.median(spread[:, e - f0]))
    for e in (109, 110, 111):  # inside what the builds span over the replicates of this table
        g = gpu[:, e - f0]
        assert g.min() >= lo[:, e - f0].min() and g.max() <= hi[:, e - f0].max(), (e, g.min(), g.max(), lo[:, e - f0].min(), hi[:, e - f0].max())
    rel109 = np.abs(gpu[:, 109 - f0] - stock[:, 109 - f0]) / stock[:, 109 - f0]
    assert np.median(rel109) <= 3.0 * np.median(spread[:, 109 - f0]), (np.median(rel109), np.median(spread[:, 109 - f0]))
    assert (ca.unresolved_epochs(fl1) >= 122 - 106).all()  # ... and the kernel says so: everything from 106 on is flagged
