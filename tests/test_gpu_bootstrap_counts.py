"""GPU: bootstrap_kernel and bootstrap_groups_kernel (colate_amd/csrc/bootstrap_kernel.hip) at their edges and in every
row shard, against the plain float64 model of bootstrap_counts_lib.py (which test_bootstrap_counts_cpu.py pins to the
oracle, to the host twin and to exact arithmetic).  The contract is an order of operations, so every comparison is bit for
bit; no tolerance appears in this file.  The largest launch is G * B = 30 workgroups."""
import ctypes

import numpy as np
import pytest

import bootstrap_counts_lib as bl
import oracle_lib as ol

pytestmark = pytest.mark.gpu
EM_KW = dict(max_iter=40, min_iter=10)  # (a short fit: the EM is only ever compared with itself on equal inputs)


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    assert colate_amd.device_count() >= 1
    return colate_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _launch_case(ca, torch, c):
    """One bootstrap_counts_device launch of a case: everything goes up in one copy.  Returns (status[1], out[2][B][A]) on
    the device; nothing is waited for."""
    A, nb, B = c.A, c.nb, c.weights.shape[0]
    host = np.concatenate([c.grid, c.weights.ravel()] + [t.ravel() for t in c.tabs])
    d = torch.from_numpy(host).to("cuda")
    grid, w = d[:A], d[A:A + B * nb].view(B, nb)
    t0 = A + B * nb
    tabs = [d[t0 + k * nb * A:t0 + (k + 1) * nb * A].view(nb, A) for k in range(4)]
    assert t0 + 4 * nb * A == d.numel()
    out = torch.full((2, B, A), float("nan"), dtype=torch.float64, device="cuda")
    status = ca.bootstrap_counts_device(grid, c.age, w, *tabs, out[0], out[1])
    return status, out


@pytest.mark.parametrize("A", bl.A_VALUES)
def test_edge_matrix_bit_identical_to_model(ca, torch, A):
    """Every in-grid case of the matrix at this A (all grids, ages, table kinds and nb; 2772 over the ten values of A):
    status 0 and both count tables equal to the model in every bit."""
    cases, model = bl.in_grid_cases(A), bl.matrix_model(A)
    assert len(cases) == len(model) == len(bl.grid_kinds(A)) * 108 - (36 if A == 2 else 0)
    runs = [_launch_case(ca, torch, c) for c in cases]
    status = torch.cat([s for s, _ in runs]).cpu().numpy()
    out = torch.stack([o for _, o in runs]).cpu().numpy()
    bad = []
    for i, c in enumerate(cases):
        m_sh, m_ns, _ = model[c.key]
        if status[i] != 0 or not np.array_equal(out[i, 0], m_sh) or not np.array_equal(out[i, 1], m_ns):
            rows, bins = np.nonzero((out[i, 0] != m_sh) | (out[i, 1] != m_ns))
            bad.append((c, int(status[i]), rows[:4].tolist(), bins[:4].tolist()))
    assert not bad, (len(bad), len(cases), bad[:6])
    print("edge matrix A=%d: %d cases" % (A, len(cases)))


def test_matrix_case_count():
    assert bl.assert_matrix_counts() == 2772 == sum(len(bl.in_grid_cases(A)) for A in bl.A_VALUES)


def test_outside_the_grid_sets_status_and_does_not_stick(ca, torch):
    """Every "outside" case (age below grid[0], on or beyond grid[A-1]) returns status 1 from bootstrap_counts_device; the
    host-pointer calls fail with the host twin's message, and the next in-grid call on the same workspace is clean."""
    cases = bl.outside_cases()
    runs = [_launch_case(ca, torch, c) for c in cases]
    status = torch.cat([s for s, _ in runs]).cpu().numpy()
    assert (status == 1).all(), [c for c, s in zip(cases, status) if s != 1]
    ep, _ = ol.epochs_from_bins("3,6.5,0.5")
    good = {A: next(c for c in bl.in_grid_cases(A) if c.tables == "dense" and c.nb == 9 and c.grid_kind == "rand") for A in (2, 65, 185)}
    for c in cases[bl.N_MATRIX_OUTSIDE - 2:]:  # two of the matrix's own and the explicit ones at A = 2, 65, 185
        with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
            ca.bootstrap_em_batch(c.grid, c.age, c.weights[:3], *c.tabs, ep, **EM_KW)
        g = good[c.A]
        out = ca.bootstrap_em_batch(g.grid, g.age, g.weights[:3], *g.tabs, ep, want_counts=True, **EM_KW)
        m_sh, m_ns, _ = bl.matrix_model(c.A)[g.key]
        assert np.array_equal(out[4], m_sh[:3]) and np.array_equal(out[5], m_ns[:3]), (c, g)
    for name in bl.GROUPS_GRIDS:
        bad, p = bl.groups_problem(name, 3, outside=True), bl.groups_problem(name, 3)
        with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
            ca.bootstrap_em_batch_groups(bad.grid, bad.ages, bad.weights, bad.tabs, bad.epochs(), **EM_KW)
        out = ca.bootstrap_em_batch_groups(p.grid, p.ages, p.weights, p.tabs, p.epochs(), want_counts=True, **EM_KW)
        assert np.array_equal(out[4], p.csh) and np.array_equal(out[5], p.cns), name


@pytest.mark.parametrize("A", [1, 257])
def test_grid_sizes_outside_the_limits_are_refused(ca, torch, A):
    """A = 1 and A = 257 are refused by the argument checks, in front of any launch: the outputs keep what they held."""
    f64 = dict(dtype=torch.float64, device="cuda")
    grid = np.sort(np.random.default_rng(A).uniform(0, 1e4, A))
    grid[0] = 0.0
    age = 0.0 if A > 1 else -1.0
    w, tab = np.ones((2, 3)), np.ones((3, A))
    out = torch.full((2, 2, A), -7.0, **f64)
    with pytest.raises(ca.ColateError, match="bad sizes"):
        ca.bootstrap_counts_device(torch.tensor(grid, **f64), age, torch.tensor(w, **f64), *(torch.tensor(tab, **f64) for _ in range(4)),
                                   out[0], out[1])
    nb, boff, age_g = torch.tensor([3], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, **f64)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ca.ColateError, match="bad sizes"):
        ca.bootstrap_counts_groups_device(1, 2, 0, 0, 2, torch.tensor(grid, **f64), nb, boff, boff, age_g, torch.tensor(w, **f64),
                                          *(torch.tensor(tab, **f64) for _ in range(4)), out[0], out[1], status)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and int(status.item()) == 0
    ep, _ = ol.epochs_from_bins("3,6.5,0.5")
    for call in (lambda: ca.bootstrap_em_batch(grid, age, w, tab, tab, tab, tab, ep, **EM_KW),
                 lambda: ca.bootstrap_em_batch_groups(grid, [age], [w], [(tab,) * 4], ep, **EM_KW),
                 lambda: ca.bootstrap_em_batch_sharded([0, 0], grid, age, w, tab, tab, tab, tab, ep, **EM_KW),
                 lambda: ca.bootstrap_em_batch_groups_sharded([0, 0], grid, [age], [w], [(tab,) * 4], ep, **EM_KW)):
        with pytest.raises(ca.ColateError, match="bad sizes" if A == 1 else "above compiled limits"):
            call()


# ---- the groups problem ----------------------------------------------------------------------------------------------
class _DeviceGroups:
    """The groups problem resident on the device, as bench.py's Workload and enqueue_rows hold a range of groups: the
    concatenated arrays of all groups once, a shard's arrays as views of them."""

    def __init__(self, torch, p):
        self.torch, self.p = torch, p
        nb, boff, woff, ages, w, tabs = p.concatenated()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        self.grid, self.nb, self.boff, self.woff, self.ages, self.w = (dev(a) for a in (p.grid.copy(), nb, boff, woff, ages, w))
        self.tabs = [dev(t) for t in tabs]
        self.h_boff, self.h_woff = boff, woff

    def launch(self, ca, lo, hi):
        """Rows [lo, hi) with the group arrays of groups lo // B .. (hi - 1) // B only, offsets relative to the first of
        them, tables and weights starting at that group, group_first = lo // B.  Returns (status, csh, cns) on the host."""
        torch, p = self.torch, self.p
        g_lo, g_hi = lo // p.B, (hi - 1) // p.B + 1
        b0, w0 = int(self.h_boff[g_lo]), int(self.h_woff[g_lo])
        b1 = int(self.h_boff[g_hi - 1]) + int(p.nb[g_hi - 1])
        boff, woff = (self.boff[g_lo:g_hi] - b0).contiguous(), (self.woff[g_lo:g_hi] - w0).contiguous()
        out = torch.full((2, hi - lo, p.A), float("nan"), dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        ca.bootstrap_counts_groups_device(g_hi - g_lo, p.B, g_lo, lo, hi, self.grid, self.nb[g_lo:g_hi], boff, woff, self.ages[g_lo:g_hi],
                                          self.w[w0:b1 * p.B], *(t[b0:b1] for t in self.tabs), out[0], out[1], status)
        return status, out


def _rows_equal(got, want, ok):
    return np.array_equal(got[ok], want[ok])


@pytest.mark.parametrize("grid_name", bl.GROUPS_GRIDS)
def test_groups_whole_range_equals_model(ca, torch, grid_name):
    """bootstrap_counts_groups_device over all rows and bootstrap_em_batch_groups(want_counts=True): row by row the model,
    for B = 1, 3, 5; with one group's age outside the grid, status 1 and every other group's rows still the model's."""
    for B in bl.GROUPS_B:
        for outside in (False, True):
            p = bl.groups_problem(grid_name, B, outside)
            status, out = _DeviceGroups(torch, p).launch(ca, 0, p.R)
            out = out.cpu().numpy()
            assert int(status.item()) == int(outside), (B, outside)
            assert _rows_equal(out[0], p.csh, p.row_ok) and _rows_equal(out[1], p.cns, p.row_ok), (B, outside)
        p = bl.groups_problem(grid_name, B)
        res = ca.bootstrap_em_batch_groups(p.grid, p.ages, p.weights, p.tabs, p.epochs(), want_counts=True, **EM_KW)
        assert np.array_equal(res[4], p.csh) and np.array_equal(res[5], p.cns), B


@pytest.mark.parametrize("grid_name", bl.GROUPS_GRIDS)
def test_groups_every_shard_of_a_world(ca, torch, grid_name):
    """Rows [lo, hi) of colate_shard_bounds for world = 2, 3, 4, 7 and G * B, launched with the shard's own group arrays:
    output rows 0 .. hi - lo equal rows lo .. hi of the whole-range result in every bit, cuts inside groups included, and
    only the shards that hold rows of the out-of-grid group report status 1."""
    from colate_amd._lib import lib

    for B in bl.GROUPS_B:
        for outside in (False, True):
            p = bl.groups_problem(grid_name, B, outside)
            dg = _DeviceGroups(torch, p)
            _, whole = dg.launch(ca, 0, p.R)
            whole = whole.cpu().numpy()
            assert _rows_equal(whole[0], p.csh, p.row_ok) and _rows_equal(whole[1], p.cns, p.row_ok)
            runs, starts_inside, ends_inside = [], 0, 0
            for world in (2, 3, 4, 7, p.R):
                covered = 0
                for rank in range(world):
                    lo_c, hi_c = ctypes.c_int(), ctypes.c_int()
                    lib.colate_shard_bounds(p.R, world, rank, ctypes.byref(lo_c), ctypes.byref(hi_c))
                    lo, hi = lo_c.value, hi_c.value
                    assert (lo, hi) == bl.shard_bounds(p.R, world, rank) and lo == covered
                    covered = hi
                    if hi == lo:
                        assert world > p.R  # (7 ranks over 6 rows: the rank has nothing to launch)
                        continue
                    starts_inside += lo % B != 0
                    ends_inside += hi % B != 0
                    runs.append((world, rank, lo, hi) + dg.launch(ca, lo, hi))
                assert covered == p.R
            if B == 5:
                assert starts_inside > 0 and ends_inside > 0
                assert any(w in (4, 7) and lo % B != 0 for w, _, lo, _, _, _ in runs)
                assert any(w in (4, 7) and hi % B != 0 for w, _, _, hi, _, _ in runs)
            status = torch.cat([r[4] for r in runs]).cpu().numpy()
            for (world, rank, lo, hi, _, out), st in zip(runs, status):
                out = out.cpu().numpy()
                what = (grid_name, B, outside, world, rank, lo, hi)
                # (rows of the out-of-grid group hold its plain sums in both runs: the same doubles, compared as well)
                assert np.array_equal(out[0], whole[0][lo:hi]) and np.array_equal(out[1], whole[1][lo:hi]), what
                holds_outside = outside and not p.row_ok[lo:hi].all()
                assert int(st) == int(holds_outside), what


@pytest.mark.parametrize("A", [3, 64, 65, 256])
def test_bootstrap_into_em_at_other_grid_sizes(ca, A):
    """bootstrap_em_batch(want_counts=True) on random grids: counts equal to the model, and rates, iterations,
    log-likelihood and flags equal in every bit to em_batch on the model's counts -- the same kernel on equal inputs."""
    c = next(c for c in bl.matrix_cases(A) if c.key == (A, "rand", 1, "dense", 9))
    ep, _ = ol.epochs_from_bins("3,6.5,0.5")
    w = c.weights[:3]
    m_sh, m_ns, _ = bl.model_counts(c.grid, c.age, w, c.tabs)
    r, it, ll, fl, csh, cns = ca.bootstrap_em_batch(c.grid, c.age, w, *c.tabs, ep, max_iter=30, want_counts=True)
    assert np.array_equal(csh, m_sh) and np.array_equal(cns, m_ns)
    r0, it0, ll0, fl0 = ca.em_batch(c.grid, m_sh, m_ns, ep, max_iter=30)
    assert np.array_equal(r, r0, equal_nan=True) and np.array_equal(ll, ll0, equal_nan=True)
    assert np.array_equal(it, it0) and np.array_equal(fl, fl0)
    assert (it0 > 0).all()  # (the fit ran; replicates 0 and 1 of the matrix are multinomial, 2 is all ones)


# ---- device lists ----------------------------------------------------------------------------------------------------
DEVICE_LISTS = ([0], [0, 0], [0] * 4, [0] * 7)


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("grid_name", bl.GROUPS_GRIDS)
def test_groups_sharded_over_device_lists(ca, grid_name):
    """colate_bootstrap_em_batch_groups_sharded with repeated ordinals (every shard its own store and stream on GPU 0;
    4 and 7 shards of 30 rows cut inside groups): all six outputs equal to the single-launch call's in every bit, the
    counts equal to the model; an out-of-grid group fails the whole call with the same message."""
    p = bl.groups_problem(grid_name, 5)
    ep = p.epochs()
    one = ca.bootstrap_em_batch_groups(p.grid, p.ages, p.weights, p.tabs, ep, want_counts=True, **EM_KW)
    assert np.array_equal(one[4], p.csh) and np.array_equal(one[5], p.cns)
    bad = bl.groups_problem(grid_name, 5, outside=True)
    for devs in DEVICE_LISTS:
        got = ca.bootstrap_em_batch_groups_sharded(devs, p.grid, p.ages, p.weights, p.tabs, ep, want_counts=True, **EM_KW)
        assert _same(got, one), devs
        assert _same(ca.bootstrap_em_batch_groups_sharded(devs, p.grid, p.ages, p.weights, p.tabs, ep, **EM_KW), one[:4]), devs
        with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
            ca.bootstrap_em_batch_groups_sharded(devs, bad.grid, bad.ages, bad.weights, bad.tabs, bad.epochs(), **EM_KW)
    after = ca.bootstrap_em_batch_groups(p.grid, p.ages, p.weights, p.tabs, ep, want_counts=True, **EM_KW)
    assert _same(after, one)


def test_genome_sharded_over_device_lists(ca):
    """colate_bootstrap_em_batch_sharded: one genome problem, B = 11 replicates of nb = 9 blocks (a shard's weights start
    at row lo; the tables are whole on every shard)."""
    c = next(c for c in bl.matrix_cases(185) if c.key == (185, "ref", 3, "dense", 9))
    w = ca.bootstrap_weights(ca.Rng(99), 11, 9)
    ep, _ = ol.epochs_from_bins("3,7,0.2")
    m_sh, m_ns, _ = bl.model_counts(c.grid, c.age, w, c.tabs)
    one = ca.bootstrap_em_batch(c.grid, c.age, w, *c.tabs, ep, want_counts=True, **EM_KW)
    assert np.array_equal(one[4], m_sh) and np.array_equal(one[5], m_ns)
    for devs in DEVICE_LISTS:
        got = ca.bootstrap_em_batch_sharded(devs, c.grid, c.age, w, *c.tabs, ep, want_counts=True, **EM_KW)
        assert _same(got, one), devs
        with pytest.raises(ca.ColateError, match=bl.OUTSIDE_MESSAGE):
            ca.bootstrap_em_batch_sharded(devs, c.grid, 2.0 * c.grid[-1], w, *c.tabs, ep, **EM_KW)
    with pytest.raises(ca.ColateError, match="out of range"):
        ca.bootstrap_em_batch_sharded([0, ca.device_count()], c.grid, c.age, w, *c.tabs, ep, **EM_KW)
