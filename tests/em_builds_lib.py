"""Runs a few replicates through every build of the EM kernel a batch size can select (csrc/em_build.hpp) and holds the builds to
each other, byte for byte, and to the oracle.  TEST INFRASTRUCTURE ONLY.

Which instantiation a replicate lands in depends on how many other replicates are in the launch: alone on a CU, two workgroups on
a CU, or the two-wave layout beyond twice the CU count.  `through_every_build` makes those launches from the same K <= 4
replicates, tiled and cut to exactly B rows; the batch sizes come from asking the library (colate_em_kernel_build), not from a
CU count written down here, and every run asserts the name of the build it took."""
import numpy as np

import oracle_lib as ol

RATE_RTOL = 1e-6  # north_star: the tolerance of every oracle comparison of the suite
LL_RTOL = 1e-11
VARIANTS = ("latency-ilp", "latency", "throughput")
NAMES = ("rates", "iterations", "loglik", "flags")
SCAN_LIMIT = 4096  # (an MI355X has 256 CUs: the edges are at 257 and 513)

REACHED = set()  # the names of the builds the runs of this process launched
CASES_RUN = 0    # ... and how many calls of through_every_build got as far as launching all of theirs


def shape_of(E):
    """NCHxEROWS of the instantiations: epochs per lane, and 16-lane rows of epochs at one epoch per lane."""
    if E <= 16:
        return "1x1"
    if E <= 32:
        return "1x2"
    if E <= 64:
        return "1x4"
    return "2x4" if E <= 128 else ("4x4" if E <= 256 else ("8x4" if E <= 512 else "16x4"))


def batch_edges(ca, E):
    """(smallest B whose build is a capped one of the max-ilp unit with the workgroups sharing CUs, largest such B, first B beyond):
    found by asking the library upward from 1.  The first comes from an epoch count that has a free build (min(E, 64): from 65
    epochs on every latency build is a capped one, whatever the batch), the third from one where the throughput layout is a choice
    (min(E, 128)).  None, None where E has no latency build."""
    first_capped = next(B for B in range(1, SCAN_LIMIT) if "capped" in ca.em_kernel_build(B, min(E, 64)))
    beyond = next((B for B in range(1, SCAN_LIMIT) if ca.em_kernel_variant(B, min(E, 128)) == "throughput"), SCAN_LIMIT)
    assert first_capped > 1, ("the library names a capped build for a batch of one replicate: it could not ask the device for its CU "
                              "count (colate_em_kernel_build_for with cus = 0), and no batch size then selects the free build or the "
                              "throughput layout -- these tests need a device that answers", ca.em_kernel_build(1, min(E, 64)))
    assert first_capped < beyond - 1, ("the batch sizes of the capped build, as the library names them, are not a range",
                                       first_capped, beyond)
    if E > 128:
        return None, None, beyond
    assert "capped" in ca.em_kernel_build(first_capped, E) and "capped" in ca.em_kernel_build(beyond - 1, E)
    return first_capped, beyond - 1, beyond


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def oracle_of(grid, csh, cns, ep, init, rows, **kw):
    """The oracle's (rates, iterations, loglik, flags) and its stable mask for the K replicates; with rows=True `ep` and `init`
    are [K][E] and every replicate is its own call."""
    if not rows:
        okw = dict(kw) if init is None else dict(kw, init=init)
        out = ol.em_batch(grid, csh, cns, ep, **okw)
        return out, ol.stable_mask(grid, csh, cns, ep, out[0], **okw)
    outs, masks = [], []
    for k in range(csh.shape[0]):
        okw = dict(kw) if init is None else dict(kw, init=init[k])
        o = ol.em_batch(grid, csh[k:k + 1], cns[k:k + 1], ep[k], **okw)
        outs.append(o)
        masks.append(ol.stable_mask(grid, csh[k:k + 1], cns[k:k + 1], ep[k], o[0], **okw))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(4)), np.concatenate(masks)


def through_every_build(ca, grid, csh, cns, ep, init=None, rows=False, floor=None, parity=True, **kw):
    """K <= 4 distinct replicates through
        the automatic build at B = K, the three forced variants at B = K,
        the automatic build at the smallest and at the largest B at which two workgroups share a CU (a capped build),
        the automatic build at the first B beyond (the throughput layout).
    Asserts: the name of the build each run took; every copy of a replicate equals its first copy and every build equals the
    automatic small batch, byte for byte, in rates, iterations, log-likelihood and flags; the K replicates agree with the oracle
    -- equal iterations and status flags, log-likelihood within LL_RTOL, rates within RATE_RTOL on the epochs the checker finds
    pinned in the oracle itself (oracle_lib.stable_mask), which must be more than `floor` of all.  kw: max_iter, min_iter,
    rel_tol.  ca=None computes the oracle's side only (for measuring `floor` without a device).  parity=False: the builds
    against each other only, for an input on which the checker cannot pin the oracle (returns the small batch's outputs alone).
    Returns (outputs of the automatic small batch, the oracle's, the mask)."""
    K, E = csh.shape[0], ep.shape[-1]
    assert K <= 4 and cns.shape == csh.shape
    if rows:
        assert ep.shape == (K, E) and init.shape == (K, E)
    if parity:
        (r0, it0, ll0, fl0), mask = oracle_of(grid, csh, cns, ep, init, rows, **kw)
        assert not (fl0 & 3).any(), "the reference aborts on this input: not a case"
        print(f"E={E} A={grid.size} {kw}: stable fraction {mask.mean():.4f}")
        if ca is None:
            return None, (r0, it0, ll0, fl0), mask
        # (a case whose oracle leaves more than a fifth of its epochs out is the wrong input, whatever its floor says)
        assert floor is not None and mask.mean() > floor and mask.mean() >= 0.8, (floor, mask.mean())

    first_capped, last_capped, beyond = batch_edges(ca, E)
    auto_name = ca.em_kernel_build(K, E)
    assert K < (first_capped or beyond)
    runs = [("automatic", K, None)] + [(v, K, v) for v in VARIANTS]
    if first_capped is not None:
        runs += [("first capped batch", first_capped, None), ("last capped batch", last_capped, None)]
    runs.append(("first batch beyond", beyond, None))

    def launch(B, forced):
        idx = np.arange(B) % K
        ca.em_force_variant(forced)
        try:
            name = ca.em_kernel_build(B, E)
            if forced is not None and E <= 128:
                assert ca.em_kernel_variant(B, E) == forced
            if rows:
                out = ca.em_batch_rows(grid, csh[idx], cns[idx], ep[idx], init[idx], **kw)
            else:
                out = ca.em_batch(grid, csh[idx], cns[idx], ep, init_rates=init, **kw)
        finally:
            ca.em_force_variant(None)
        REACHED.add(name)
        return name, idx, out

    first = None
    for label, B, forced in runs:
        name, idx, out = launch(B, forced)
        # the build the run took: its kind by where the batch size lies, its shape by the epoch count
        assert name.endswith("/" + shape_of(E)), (label, name)
        if E > 128:
            want = "default-tput"
        elif label == "automatic":
            want = "ilp-free" if E <= 64 else "ilp-capped"
        elif forced is not None:
            want = {"latency-ilp": auto_name.split("/")[0], "latency": "default-capped", "throughput": "default-tput"}[forced]
        else:
            want = "default-tput" if B == beyond else "ilp-capped"
        assert name.split("/")[0] == want, (label, B, name, want)
        for what, a in zip(NAMES, out):
            assert a.shape[0] == B
            for k in range(K):  # every copy of a replicate equals the first
                copies = a[idx == k]
                assert _bits(copies) == _bits(np.broadcast_to(copies[:1], copies.shape)), (label, name, what, k)
        head = tuple(a[:K] for a in out)
        if first is None:
            first = head
        for what, a, b in zip(NAMES, first, head):  # every build equals the automatic small batch
            assert _bits(a) == _bits(b), (label, name, what)

    if not parity:
        return first
    global CASES_RUN
    CASES_RUN += 1
    r, it, ll, fl = first
    rel = np.abs(r - r0) / np.maximum(np.abs(r0), 1e-300)
    print(f"  against the oracle: loglik rel diff {np.max(np.abs(ll - ll0) / np.abs(ll0)):.2e}, rates rel diff on the stable epochs "
          f"{rel[mask].max(initial=0.0):.2e}, iterations {it.tolist()} / {it0.tolist()}")
    assert (it == it0).all(), (it, it0)
    assert (ca.status_flags(fl) == fl0).all(), (fl, fl0)
    assert np.allclose(ll, ll0, rtol=LL_RTOL, atol=0), (ll, ll0)
    assert rel[mask].max(initial=0.0) < RATE_RTOL, (float(rel[mask].max(initial=0.0)), mask.mean())
    return first, (r0, it0, ll0, fl0), mask

