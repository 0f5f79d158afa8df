"""The cases of the count bootstrap (bootstrap_kernel / bootstrap_groups_kernel, coal.cpp:3358-3441) and a plain NumPy
model of one replicate.  TEST INFRASTRUCTURE ONLY: shared by test_bootstrap_counts_cpu.py and test_gpu_bootstrap_counts.py.

The contract of the kernels is an order of operations -- blocks ascending, bins ascending, every product rounded and then
added -- so the model restates that order in float64 and every comparison with it is `array_equal`: no tolerance anywhere.
The model shares no code with the product or with oracle/colate_oracle.c; the CPU test pins it to both and to exact
arithmetic.

The edge matrix (issue "Test the count bootstrap kernels at their edges and in every row shard"):
  A      2, 3, 63, 64, 65, 128, 129, 185, 255, 256   (the launch is (A + 63) & ~63 threads, LDS arrays of 256)
  grid   "ref" the reference grid's first A bins (A <= 185) | "rand" sorted log-uniform | "dup" rand with two equal
         neighbours in the middle, grid[A//2 - 1] == grid[A//2] (A >= 4)
  age    0 grid[0] | 1 midway through the first cell | 2 grid[A//2] exactly | 3 one ulp below grid[A//2] | 4 grid[A-2] |
         5 one ulp below grid[A-1]
  nb     1, 2, 9
  tables dense | noemp | emp_below | emp_last | emp_shonly | skipinf
  B = 4 replicates per case: two multinomial rows, the all-ones row of num_bootstrap == 1, an all-zero row.
26 grids x 6 ages x 3 nb x 6 table kinds = 2808 cases.  In 36 of them the age lies outside the grid (A = 2, where grid[A//2]
is the last bin): those are not dropped, they join the "outside" cases; 2772 are in-grid.  Both numbers are asserted below.
`skipinf` at nb = 1 has one block, which has weight 0 in every replicate like block 0 at nb >= 2: all four replicates are
zero-weight there."""
import functools
import math

import numpy as np

import oracle_lib as ol

A_VALUES = (2, 3, 63, 64, 65, 128, 129, 185, 255, 256)
GRID_KINDS = ("ref", "rand", "dup")
N_AGES = 6
NB_VALUES = (1, 2, 9)
TABLE_KINDS = ("dense", "noemp", "emp_below", "emp_last", "emp_shonly", "skipinf")
B_MATRIX = 4
ZERO_REPLICATE = 3  # (row of the all-zero weights; row 2 is all ones)
N_MATRIX, N_MATRIX_IN_GRID, N_MATRIX_OUTSIDE = 2808, 2772, 36
OUTSIDE_MESSAGE = "sample age outside the age grid"


# ---- the model -------------------------------------------------------------------------------------------------------
class Replicate:
    """What model_replicate found: outside (bool), bin_start, the four weighted sums, fcount, F after the scaling, normf and
    the two count rows (csh, cns; None when outside)."""


def model_replicate(grid, age, w, sh, ns, she, nse):
    """One replicate: w[nb], four tables [nb][A].  Blocks ascending with w[j] <= 0 skipped, product then sum; bin_start by
    searchsorted; fcount, F, the scaling by the cell widths (lower_age trailing one bin) and normf bins ascending."""
    grid = np.asarray(grid, dtype=np.float64)
    A, nb = grid.size, len(w)
    sums = [np.zeros(A) for _ in range(4)]
    for j in range(nb):
        if w[j] <= 0:
            continue
        for k, t in enumerate((sh, ns, she, nse)):
            sums[k] = sums[k] + w[j] * t[j]
    r = Replicate()
    r.sums = sums
    r.bin_start = int(np.searchsorted(grid, age, side="right"))
    r.outside = r.bin_start < 1 or r.bin_start >= A
    r.csh = r.cns = None
    if r.outside:
        return r
    g, e_sh, e_ns = grid.tolist(), sums[2].tolist(), sums[3].tolist()  # (Python floats are the same IEEE doubles)
    fcount, F = 0.0, [0.0] * A
    for b in range(r.bin_start, A):
        fcount += e_sh[b]
        if e_sh[b] > 0:
            F[b] = e_sh[b] / (e_sh[b] + e_ns[b])
    lower_age = g[r.bin_start - 1]
    for b in range(r.bin_start, A):
        F[b - 1] *= g[b] - lower_age
        lower_age = g[b]
    normf = 0.0
    for b in range(A):
        normf += F[b]
    r.fcount, r.F, r.normf = fcount, np.array(F), normf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        add = r.F / np.float64(normf) * np.float64(fcount)
    r.csh = sums[0] + np.where(add > 0, add, 0.0)  # max(0.0, NaN) == 0.0
    r.cns = sums[1]
    return r


def model_counts(grid, age, weights, tabs):
    """All replicates of weights[B][nb]: (csh[B][A], cns[B][A], [Replicate]); the arrays are None if the age is outside."""
    reps = [model_replicate(grid, age, w, *tabs) for w in np.atleast_2d(weights)]
    if reps[0].outside:
        return None, None, reps
    return np.stack([r.csh for r in reps]), np.stack([r.cns for r in reps]), reps


def plain_bin_start(grid, age):
    """How many grid points are <= age, counted one by one (the intended bin_start of a case, without searchsorted)."""
    return sum(1 for x in np.asarray(grid).tolist() if x <= age)


def exact_sum_bound(w, table):
    """(fsum[A], bound[A]): math.fsum of the exact products w[j] * table[j][b] over the blocks with w[j] > 0, and
    nb * 2**-53 * sum_j |w[j] * table[j][b]|.  The products are exact because each table entry is split into two halves of
    at most 27 bits (Veltkamp) and the weights are integers below 2**8.  The bound is that of a recursive inner product of
    length nb in round-to-nearest, |fl(x.y) - x.y| <= nb * u * |x|.|y| with u = 2**-53 and no higher-order term
    (Jeannerod and Rump, "Improved error bounds for inner products in floating-point arithmetic", SIAM J. Matrix Anal.
    Appl. 34, 2013): derived, not measured."""
    w, table = np.asarray(w, dtype=np.float64), np.asarray(table, dtype=np.float64)
    nb, A = table.shape
    live = w > 0
    w, table = w[live], table[live]
    assert np.isfinite(table).all() and (w == np.rint(w)).all() and (w < 256).all()
    c = 134217729.0 * table  # 2**27 + 1
    hi = c - (c - table)
    lo = table - hi
    assert (hi + lo == table).all()
    terms = np.concatenate([w[:, None] * hi, w[:, None] * lo, np.zeros((1, A))])  # every product exact
    exact = np.array([math.fsum(col) for col in terms.T.tolist()])
    bound = nb * 2.0 ** -53 * np.array([math.fsum(col) for col in np.abs(terms).T.tolist()])
    return exact, bound


# ---- the edge matrix -------------------------------------------------------------------------------------------------
def grid_kinds(A):
    return tuple(k for k in GRID_KINDS if (k != "ref" or A <= 185) and (k != "dup" or A >= 4))


@functools.lru_cache(maxsize=None)
def make_grid(A, kind):
    if kind == "ref":
        g = ol.age_grid()[:A].copy()
    else:
        rng = np.random.default_rng(1000 + A)
        g = np.sort(np.exp(rng.uniform(np.log(2.0), np.log(4e5), A)))
        if kind == "dup":
            g[A // 2 - 1] = g[A // 2]
    assert g.size == A and (np.diff(g) >= 0).all()
    g.setflags(write=False)
    return g


def case_age(grid, ai):
    A = grid.size
    return [grid[0], 0.5 * (grid[0] + grid[1]), grid[A // 2], np.nextafter(grid[A // 2], 0.0), grid[A - 2],
            np.nextafter(grid[A - 1], 0.0)][ai].item()


def intended_bin_start(A, kind, ai):
    """bin_start of the six ages by construction (`dup`: grid[h - 1] == grid[h], h = A // 2, so the grid point skips both
    and one ulp below it stops in front of both)."""
    h = A // 2
    return [1, 1, h + 1, h - 1 if kind == "dup" else h, A - 1, A - 1][ai]


@functools.lru_cache(maxsize=None)
def _base_tables(A, nb, seed):
    rng = np.random.default_rng(seed)
    sh = rng.uniform(0, 3, (nb, A)) * (rng.uniform(size=(nb, A)) < 0.6)
    ns = rng.uniform(0, 9, (nb, A)) * (rng.uniform(size=(nb, A)) < 0.6)
    she = rng.uniform(0, 1, (nb, A)) * (rng.uniform(size=(nb, A)) < 0.7)
    nse = rng.uniform(0, 1, (nb, A)) * (rng.uniform(size=(nb, A)) < 0.7)
    last = rng.uniform(0.1, 1, nb)
    return sh, ns, she, nse, last


def make_tables(A, nb, kind, bin_start, seed=None):
    """(sh, ns, she, nse), each [nb][A].  `bin_start` is where the age of the case falls (emp_below cuts there)."""
    sh, ns, she, nse, last = (x.copy() for x in _base_tables(A, nb, 7 * A + nb if seed is None else seed))
    if kind == "noemp":
        she[:], nse[:] = 0.0, 0.0
    elif kind == "emp_below":
        she[:, max(bin_start, 0):] = 0.0  # nothing at or above bin_start: fcount = 0, every F = 0, normf = 0
    elif kind == "emp_last":
        she[:] = 0.0
        she[:, A - 1] = last  # every block: any replicate with a positive weight has she[A-1] > 0
    elif kind == "emp_shonly":
        nse[:] = 0.0  # F = 1 wherever she > 0
    elif kind == "skipinf":
        sh[0, A // 3] = np.inf  # block 0 has weight 0 in every replicate: 0 * inf and 0 * nan must never be formed
        she[0, A - 1] = np.nan
    else:
        assert kind == "dense"
    return sh, ns, she, nse


@functools.lru_cache(maxsize=None)
def _matrix_weights(nb, skip_block0):
    """[4][nb]: two multinomial rows (nb draws over the blocks), all ones, all zero; skip_block0: no draw ever lands on block
    0 and its weight is 0 in every row."""
    rng = np.random.default_rng(50 + nb + 100 * skip_block0)
    w = np.zeros((B_MATRIX, nb))
    first = 1 if skip_block0 else 0
    live = nb - first
    for i in range(2):
        if live:
            w[i, first:] = rng.multinomial(nb, np.full(live, 1.0 / live))
    w[2, first:] = 1.0
    assert (w[ZERO_REPLICATE] == 0).all()
    w.setflags(write=False)
    return w


class Case:
    def __init__(self, A, grid_kind, ai, tables, nb):
        self.key = (A, grid_kind, ai, tables, nb)
        self.A, self.grid_kind, self.ai, self.tables, self.nb = A, grid_kind, ai, tables, nb
        self.grid = make_grid(A, grid_kind)
        self.age = case_age(self.grid, ai)
        self.bin_start = plain_bin_start(self.grid, self.age)
        self.outside = self.bin_start < 1 or self.bin_start >= A
        self.weights = _matrix_weights(nb, tables == "skipinf")
        self.tabs = make_tables(A, nb, tables, self.bin_start)

    def __repr__(self):
        return "case(A=%d, grid=%s, age#%d=%r, tables=%s, nb=%d)" % (self.A, self.grid_kind, self.ai, self.age, self.tables, self.nb)


@functools.lru_cache(maxsize=None)
def matrix_cases(A):
    """Every case of the matrix at this A, in-grid and outside alike."""
    return tuple(Case(A, gk, ai, tk, nb) for gk in grid_kinds(A) for ai in range(N_AGES) for tk in TABLE_KINDS for nb in NB_VALUES)


def in_grid_cases(A):
    return tuple(c for c in matrix_cases(A) if not c.outside)


@functools.lru_cache(maxsize=None)
def outside_cases():
    """The matrix cases whose age fell outside the grid, plus age = -1 (bin 0), age = grid[A-1] and 2 * grid[A-1] (bin A)
    on every grid of A = 2, 65 and 185 (dense tables, nb = 9)."""
    out = [c for A in A_VALUES for c in matrix_cases(A) if c.outside]
    assert len(out) == N_MATRIX_OUTSIDE
    for A in (2, 65, 185):
        for gk in grid_kinds(A):
            g = make_grid(A, gk)
            for age, want in ((-1.0, 0), (g[A - 1].item(), A), (2.0 * g[A - 1].item(), A)):
                c = Case(A, gk, 0, "dense", 9)
                c.age, c.bin_start, c.outside, c.key = age, plain_bin_start(g, age), True, (A, gk, age, "dense", 9)
                assert c.bin_start == want
                out.append(c)
    return tuple(out)


def assert_matrix_counts():
    """The matrix holds what the module's docstring says: nothing left out, nothing skipped."""
    total = sum(len(matrix_cases(A)) for A in A_VALUES)
    inside = sum(len(in_grid_cases(A)) for A in A_VALUES)
    assert (total, inside, total - inside) == (N_MATRIX, N_MATRIX_IN_GRID, N_MATRIX_OUTSIDE), (total, inside)
    assert len(outside_cases()) == N_MATRIX_OUTSIDE + 3 * (2 + 3 + 3)
    return inside


@functools.lru_cache(maxsize=None)
def matrix_model(A):
    """{case key: (csh[4][A], cns[4][A], [Replicate])} of the in-grid cases at this A; computed once, read-only."""
    out = {}
    for c in in_grid_cases(A):
        csh, cns, reps = model_counts(c.grid, c.age, c.weights, c.tabs)
        csh.setflags(write=False), cns.setflags(write=False)
        out[c.key] = (csh, cns, reps)
    return out


# ---- the groups problem ----------------------------------------------------------------------------------------------
GROUPS_NB = (1, 9, 2, 115, 3, 16)
GROUPS_TABLES = ("dense", "noemp", "emp_below", "emp_last", "emp_shonly", "dense")
GROUPS_B = (1, 3, 5)
GROUPS_GRIDS = ("ref185", "rand65")
OUTSIDE_GROUP = 2


@functools.lru_cache(maxsize=None)
def groups_grid(name):
    if name == "ref185":
        g = ol.age_grid().copy()
        assert g.size == 185
    else:
        g = make_grid(65, "rand").copy()
        g[0] = 0.0  # (as the reference's grid: a modern sample, age 0, lies in the first cell)
    assert g[0] == 0.0 and g[1] < 250.0 < g[-2]
    g.setflags(write=False)
    return g


class Groups:
    """G = 6 groups x B replicates on one grid: per group nb, age, tables, weights[B][nb] (colate_amd.bootstrap_weights,
    one seed per group) and the model's rows.  outside=True moves group OUTSIDE_GROUP's age beyond the grid."""

    def __init__(self, grid_name, B, outside=False):
        import colate_amd as ca

        self.grid = grid = groups_grid(grid_name)
        self.A, self.B, self.G = grid.size, B, len(GROUPS_NB)
        A = self.A
        self.nb = np.array(GROUPS_NB, dtype=np.int32)
        ages = [0.0, grid[A // 3].item(), np.nextafter(grid[A // 2], 0.0).item(), grid[A - 2].item(), 250.0, 0.0]
        if outside:
            ages[OUTSIDE_GROUP] = 2.0 * grid[A - 1].item()
        self.ages = np.array(ages)
        self.outside_group = OUTSIDE_GROUP if outside else None
        self.tabs, self.weights = [], []
        for g in range(self.G):
            bs = plain_bin_start(grid, ages[g])
            self.tabs.append(make_tables(A, int(self.nb[g]), GROUPS_TABLES[g], min(bs, A), seed=1000 * (g + 1) + A))
            self.weights.append(ca.bootstrap_weights(ca.Rng(4242 + g), B, int(self.nb[g])))
        self.R = self.G * B
        self.csh, self.cns = np.full((self.R, A), np.nan), np.full((self.R, A), np.nan)
        self.row_ok = np.ones(self.R, dtype=bool)  # rows of in-grid groups
        for g in range(self.G):
            rows = slice(g * B, (g + 1) * B)
            csh, cns, _ = model_counts(grid, ages[g], self.weights[g], self.tabs[g])
            if csh is None:
                assert g == self.outside_group
                self.row_ok[rows] = False
            else:
                self.csh[rows], self.cns[rows] = csh, cns
        assert self.row_ok.sum() == self.R - (B if outside else 0)
        self.csh.setflags(write=False), self.cns.setflags(write=False)

    def epochs(self):
        """[G][E]: an epoch grid per group, two different ones among them (an ancient sample's age replaces an epoch
        boundary, the count stays); any valid epochs do for a fit that is only compared with itself."""
        ep = [ol.epochs_from_bins("3,7,0.2", 250.0 if 0.0 < a else 0.0, 28.0)[0] for a in self.ages]
        assert len({len(e) for e in ep}) == 1
        return np.stack(ep)

    def concatenated(self, g_lo=0, g_hi=None):
        """The arrays of groups [g_lo, g_hi) as a launch takes them: nb, block offsets and weight offsets relative to group
        g_lo, ages, weights and the four tables concatenated from group g_lo on."""
        g_hi = self.G if g_hi is None else g_hi
        nb = self.nb[g_lo:g_hi]
        boff = np.concatenate([[0], np.cumsum(nb[:-1])]).astype(np.int64)
        w = np.concatenate([self.weights[g].ravel() for g in range(g_lo, g_hi)])
        tabs = [np.concatenate([self.tabs[g][k] for g in range(g_lo, g_hi)]) for k in range(4)]
        return nb.copy(), boff, boff * self.B, self.ages[g_lo:g_hi].copy(), w, tabs


@functools.lru_cache(maxsize=None)
def groups_problem(grid_name, B, outside=False):
    return Groups(grid_name, B, outside)


def shard_bounds(R, world, rank):
    """The balanced contiguous split of colate_shard_bounds, restated."""
    base, rem = divmod(R, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)
