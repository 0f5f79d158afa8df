"""The age-sampling kernel of the table fill (colate_amd/csrc/fill_kernel.hip, fill_device.h) against a float64 reference written
here, kernel by kernel rather than through the CLI: colate_amd/bin/fill_kernel_check links the product's fill_kernel.o and drives
DeviceFill (make_device_fill, alloc_staging, alloc_uniforms, upload_uniforms, sync_uploads, submit, finish) over a scripted case.

The contract (fill_device.h, mut_pairs.cpp Engine::sample): for each used SNP, 100 ages x = u * span + begin (a multiply and an add,
each rounded), bin(x) = max(0, round_half_away(log(10 x) * 10) + 1) (coal.cpp:2265, 2284); the SNP's weight is added to the bin once
per sample, one addition after another, SNP after SNP in file order.  Where the kernel cannot decide -- a sample within 64 ulps of
a step (a guard band), or a sample of a non-F row (begin > 0) beyond the grid or below 0 -- it flags the table and the host fills
the pair again.  Every clean table must equal the reference bit for bit; every table with such a sample must be flagged; no other
table may be flagged."""
import functools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "colate_amd", "bin", "fill_kernel_check")
DRAWS = 100
F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
REC = np.dtype([("begin", "<f4"), ("end", "<f4"), ("w_sh", "<f8"), ("w_ns", "<f8")])  # FillRec
JOB = np.dtype([("rec_off", "<u8"), ("u_off", "<u8"), ("nrec", "<u4"), ("table", "<u4")])  # FillJob
assert REC.itemsize == 24 and JOB.itemsize == 24


# ---------------------------------------------------------------------------------------------------- the reference
def _round_half_away(v):
    t = math.trunc(v)
    if v - t >= 0.5:
        return t + 1
    if t - v >= 0.5:
        return t - 1
    return t


def age_bin(x):
    """The library expression (age_bins.hpp age_bin_index, C = 10), with the scalar libm logarithm."""
    if not x > 0.0:
        return 0  # log(0) = -inf (and log(x < 0) = nan): the reference's cast ends at max(0, .) = 0
    return max(0, _round_half_away(math.log(10 * x) * 10.0) + 1)


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


@functools.lru_cache(maxsize=None)
def guards(A):
    """(thr, lo, hi), A + 2 values each: thr[k] the smallest double with age_bin >= k (bisection over the bit patterns),
    the guard band around it [thr - 64 ulp, thr + 64 ulp); [0] = -inf, [A + 1] = +inf."""
    inf = math.inf
    thr, lo, hi = [-inf], [-inf], [-inf]
    for k in range(1, A + 1):
        a, b = _bits(1e-300), _bits(1e300)
        while b - a > 1:
            mid = a + (b - a) // 2
            if age_bin(_from_bits(mid)) >= k:
                b = mid
            else:
                a = mid
        thr.append(_from_bits(b))
        lo.append(_from_bits(b - 64))
        hi.append(_from_bits(b + 64))
    thr.append(inf), lo.append(inf), hi.append(inf)
    return np.array(thr), np.array(lo), np.array(hi)


def samples(rec, U, u0):
    begin, end = float(rec["begin"]), float(rec["end"])  # (float -> double: exact)
    span = end - begin
    u = U[u0:u0 + DRAWS]
    return u * span + begin  # (numpy: a rounded multiply, then a rounded add)


def classify(x, A):
    """(bin, in_band) per sample: bin = #{k : thr_k <= x}, checked against the library expression outside the bands."""
    thr, lo, hi = guards(A)
    b = np.searchsorted(thr[1:A + 1], x, side="right")
    k = np.searchsorted(lo[1:A + 1], x, side="right") - 1
    band = (k >= 0) & (x < hi[1:A + 1][np.maximum(k, 0)])
    for xi, bi in zip(x[~band], b[~band]):
        assert min(age_bin(float(xi)), A) == bi, (xi, bi)
    return b, band


def expected(recs, u_off, U, A, order=None):
    """(sh, ns, flag) of one job: the reference fill of a zero table."""
    sh, ns = np.zeros(A), np.zeros(A)
    flag = False
    idx = range(len(recs)) if order is None else order
    for i in idx:
        r = recs[i]
        x = samples(r, U, u_off + DRAWS * i)
        b, band = classify(x, A)
        nonf = float(r["begin"]) > 0.0
        flag = flag or bool(band.any()) or (nonf and bool((b >= A).any() or (x < 0.0).any()))
        cnt = np.bincount(b[b < A], minlength=A)
        for c in range(1, int(cnt.max(initial=0)) + 1):
            m = cnt >= c
            sh[m] += r["w_sh"]
            ns[m] += r["w_ns"]
    return sh, ns, flag


# ---------------------------------------------------------------------------------------------------- the case file
class Case:
    def __init__(self, A, max_tables, batch_recs, U):
        self.A, self.max_tables, self.batch_recs, self.U = A, max_tables, batch_recs, U
        self.max_uniforms = len(U) - DRAWS
        self.ops = []
        self.jobs = []  # (table, recs, u_off): what the reference fills
        _, lo, hi = guards(A)
        self.head = struct.pack("<iQQQ", A, max_tables, batch_recs, self.max_uniforms) + lo.astype("<f8").tobytes() + hi.astype("<f8").tobytes()

    def upload(self, off, values):
        self.ops.append(struct.pack("<IQQ", 1, off, len(values)) + np.asarray(values, dtype="<f8").tobytes())

    def sync(self):
        self.ops.append(struct.pack("<I", 2))

    def submit(self, jobs, refuse=False):
        """jobs: (table, recs, u_off) each; their records side by side in the staging buffer."""
        recs = np.concatenate([j[1] for j in jobs]) if jobs else np.zeros(0, REC)
        js = np.zeros(len(jobs), JOB)
        off = 0
        for i, (t, r, u_off) in enumerate(jobs):
            js[i] = (off, u_off, len(r), t)
            off += len(r)
            assert u_off + DRAWS * len(r) <= len(self.U)
        self.ops.append(struct.pack("<IIQQ", 3, int(refuse), len(js), len(recs)) + recs.tobytes() + js.tobytes())
        if not refuse:
            self.jobs += list(jobs)

    def finish(self):
        self.ops.append(struct.pack("<I", 4))

    def run(self, tmp_path, name="case"):
        p, o = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
        p.write_bytes(self.head + b"".join(self.ops))
        r = subprocess.run([EXE, str(p), str(o)], capture_output=True, timeout=120)
        if r.returncode != 0:
            return r, None, None
        raw = o.read_bytes()
        nt = self.max_tables * 2 * self.A * 8
        tables = np.frombuffer(raw[:nt], dtype="<f8").reshape(self.max_tables, 2, self.A)
        flags = np.frombuffer(raw[nt:], dtype="<i4")
        assert len(flags) == self.max_tables
        return r, tables, flags


def check(case, tables, flags):
    """Every expected flag set, every clean table the reference's bits, nothing else flagged (the kernel is conservative in no
    class: a flag costs the whole pair a refill on the host), untouched tables +0.0.  Returns (clean tables, flagged tables)."""
    A = case.A
    seen = set()
    clean = flagged = 0
    for t, recs, u_off in case.jobs:
        assert t not in seen  # (one job per table, as on the host)
        seen.add(t)
        sh, ns, flag = expected(recs, u_off, case.U, A)
        if flag:
            assert flags[t] == 1, f"table {t}: a sample in a guard band / beyond the grid, not flagged"
            flagged += 1
            continue
        assert flags[t] == 0, f"table {t}: flagged, but the reference decides every sample"
        assert np.array_equal(tables[t, 0].view(np.uint64), sh.view(np.uint64)), (t, np.flatnonzero(tables[t, 0] != sh)[:8])
        assert np.array_equal(tables[t, 1].view(np.uint64), ns.view(np.uint64)), (t, np.flatnonzero(tables[t, 1] != ns)[:8])
        clean += 1
    for t in range(case.max_tables):
        if t not in seen:
            assert flags[t] == 0 and not tables[t].view(np.uint64).any(), f"table {t}: no job, but touched"
    return clean, flagged


# ---------------------------------------------------------------------------------------------------- building cases
def _f32_below(v):
    b = F32(v)
    return b if float(b) < v else np.nextafter(b, F32(-np.inf))


def _u_hitting(begin, end, target, accept=None):
    """A u in [0, 1) whose sample u * span + begin (two roundings) is `target` exactly (or satisfies `accept`)."""
    begin, end = float(begin), float(end)
    span = end - begin
    u = min(max((target - begin) / span, 0.0), 1.0 - 2.0**-53)
    for _ in range(256):
        x = u * span + begin
        if (accept(x) if accept else x == target):
            assert 0.0 <= u < 1.0
            return u
        u = float(np.nextafter(u, 1.0 if x < target else 0.0))
    raise AssertionError(("no u reaches", begin, end, target))


def _host_weight(rng, f_max=2):
    """f_target * DAF_ref / (N_ref * 100) as use_snp forms it (f rounded in float, DAF_ref <= N_ref)."""
    n_ref = int(rng.integers(1, 5))
    daf = int(rng.integers(1, n_ref + 1))
    f = float(F32(int(rng.integers(0, f_max + 1))) * F32(daf))
    return f / (n_ref * 100.0)


STRESS = (1.0, 1e-16, 5e-324, 2.2e-310, 1e300)


def random_recs(rng, n, A, wide):
    """n rows, ~10 % of them F-path (begin = 0, w_sh = +0.0); ages log-uniform over [1e-3, top]: top 2e7 for `wide` jobs (beyond the
    grid: non-F rows flag), else a third of the last step (every sample on the grid)."""
    thr = guards(A)[0]
    top = 2e7 if wide else min(2e7, thr[A] / 3)
    recs = np.zeros(n, REC)
    for i in range(n):
        age = math.exp(rng.uniform(math.log(1e-3), math.log(top)))
        if rng.uniform() < 0.1:
            recs[i] = (0.0, F32(age), 0.0, _host_weight(rng))
        else:
            b = F32(age)
            e = F32(float(b) * (1 + 1.5 * rng.uniform()))
            w_sh, w_ns = _host_weight(rng), _host_weight(rng)
            if rng.uniform() < 0.03:
                w_sh, w_ns = STRESS[rng.integers(len(STRESS))], STRESS[rng.integers(len(STRESS))]
            recs[i] = (b, e, w_sh, w_ns)
    return recs


class Hand:
    """Hand-placed rows: each a job (a table) of its own, so that a flag is the row's.  `u0` places sample 0 where the row
    wants it; `flag` (where not None) and `target_bin` (sample 0's bin) are checked against the reference when the case is built."""

    def __init__(self, A, rng):
        self.A, self.rng, self.rows = A, rng, []  # (name, rec, u0 or None, flag, target_bin)

    def add(self, name, begin, end, w, u0=None, flag=None, target_bin=None):
        rec = np.zeros(1, REC)
        rec[0] = (begin, end, 0.0 if not float(F32(begin)) > 0 else w, w)
        self.rows.append((name, rec, u0, flag, target_bin))

    def around_step(self, k):
        """A float-apart (begin, end) with thr_k between them."""
        thr = guards(self.A)[0]
        b = _f32_below(thr[k])
        return b, np.nextafter(b, F32(np.inf))

    def standard(self, ks):
        A = self.A
        thr, lo, hi = guards(A)
        w = 1.0 / 300.0
        for k in ks:
            b, e = self.around_step(k)
            in_band = lambda x, k=k: lo[k] <= x < hi[k]  # noqa: E731
            self.add(f"band{k}", b, e, w, _u_hitting(b, e, thr[k], in_band), flag=True)
            self.add(f"at_lo{k}", b, e, w, _u_hitting(b, e, lo[k]), flag=True)
            self.add(f"at_hi{k}", b, e, w, _u_hitting(b, e, hi[k]), target_bin=k, flag=k == A)
            self.add(f"below_lo{k}", b, e, w, _u_hitting(b, e, float(np.nextafter(lo[k], -np.inf))), target_bin=k - 1, flag=False)
            eF = F32(min(2.0 * thr[k], FLT_MAX))
            self.add(f"band{k}_F", 0.0, eF, w, _u_hitting(0.0, eF, thr[k], in_band), flag=True)
            self.add(f"at_hi{k}_F", 0.0, eF, w, _u_hitting(0.0, eF, hi[k], lambda x, k=k: hi[k] <= x < lo[k + 1]), target_bin=k, flag=False)
        # one bin takes all 100 samples (the last bin: the highest lane of the last slot)
        b = F32(math.sqrt(thr[A - 1] * thr[A])) if A > 1 else F32(thr[1] / 2)
        self.add("one_bin_last", b, np.nextafter(b, F32(np.inf)), 0.37, target_bin=A - 1, flag=False)
        self.add("below_thr1", 1e-3, F32(lo[1] / 2), 0.01, flag=False)
        self.add("x_zero_F", 0.0, 50.0, 0.02, 0.0, target_bin=0, flag=False)
        self.add("u_max", F32(thr[A] / 4), F32(thr[A] / 2), 0.03, 1.0 - 2.0**-53)
        self.add("u_max_F", 0.0, F32(thr[A] / 2), 0.03, 1.0 - 2.0**-53)
        self.add("flt_max", 1.0, FLT_MAX, 0.01, flag=True)
        self.add("subnormal_begin", np.float32(1.4e-45), F32(lo[1] / 2), 0.01, flag=False)
        self.add("subnormal_begin_beyond", np.float32(1.4e-45), F32(min(4 * thr[A], 1e30)), 0.01, flag=True)
        self.add("beyond_F", 0.0, F32(thr[A] * 1.6), 0.05, flag=False)
        self.add("beyond_nonF", F32(thr[A] * 1.1), F32(thr[A] * 2.0), 0.05, flag=True)
        self.add("negative_nonF", 1.0, -5.0, 0.05, flag=True)

    def jobs(self, U, u_cursor, table_of):
        """Writes the rows' uniforms into U from u_cursor on; returns ((table, recs, u_off) per row, the next cursor).  A placed
        sample 0 is the row's largest (the others are below it: the row's other samples stay on the placed one's side)."""
        out = []
        for i, (name, rec, u0, flag, target_bin) in enumerate(self.rows):
            U[u_cursor:u_cursor + DRAWS] = self.rng.uniform(size=DRAWS)
            if u0 is not None:
                U[u_cursor:u_cursor + DRAWS] *= u0
                U[u_cursor] = u0
            x = samples(rec[0], U, u_cursor)
            b, band = classify(x, self.A)
            if target_bin is not None:
                assert b[0] == target_bin and not band[0], (name, b[0], band[0])
            if name.startswith("one_bin"):
                assert (b == b[0]).all() and not band.any(), name
            if name == "beyond_F":
                assert (b >= self.A).any() and (b < self.A).any(), name
            _, _, f = expected(rec, u_cursor, U, self.A)
            if flag is not None:
                assert f == flag, (name, f)
            out.append((table_of(i), rec, u_cursor))
            u_cursor += DRAWS + 2  # (odd offsets only)
        return out, u_cursor


def build_case(A, seed, n_submits, plan, batch_recs, hand_ks, extra_jobs=()):
    """The randomized jobs of `plan` (nrec per job, per submit) plus the hand-placed rows spread over the submits; tables
    scattered over a range with gaps; every u_off odd; the last row's uniforms end at max_uniforms + 100.  The second half of the
    uniforms is uploaded as sentinels first, synced, then uploaded for real and submitted on WITHOUT a sync."""
    rng = np.random.default_rng(seed)
    hand = Hand(A, rng)
    hand.standard(hand_ks)
    n_rand = sum(len(s) for s in plan)
    n_jobs = n_rand + len(hand.rows) + len(extra_jobs)
    max_tables = 2 * n_jobs + 7
    tables = rng.permutation(max_tables)[:n_jobs]  # (the rest: tables no job touches)
    total = 1 + sum(DRAWS * n + 2 for s in plan for n in s) + (DRAWS + 2) * len(hand.rows) + sum(DRAWS * len(r) + 2 for r in extra_jobs) + 10
    U = rng.uniform(size=total)
    per_submit = [[] for _ in range(n_submits)]
    cursor = 1
    hand_jobs, cursor = hand.jobs(U, cursor, lambda i: int(tables[n_rand + i]))
    for i, j in enumerate(hand_jobs):
        per_submit[(3 * i) % (n_submits // 2)].append(j)  # (the first half: the uniforms uploaded with a sync)
    ti = 0
    late_from = None
    for s, nrecs in enumerate(plan):
        if s == n_submits // 2:
            late_from = cursor
        for n in nrecs:
            recs = random_recs(rng, n, A, wide=rng.uniform() < 0.3)
            per_submit[s].append((int(tables[ti]), recs, cursor))
            ti += 1
            cursor += DRAWS * n + 2
    for i, r in enumerate(extra_jobs):
        per_submit[-1].append((int(tables[n_rand + len(hand.rows) + i]), r, cursor))
        cursor += DRAWS * len(r) + 2
    U = U[:cursor - 2]  # (the last job of the last submit ends exactly at max_uniforms + 100)
    t_last, r_last, u_last = per_submit[-1][-1]
    assert u_last % 2 == 1 and u_last + DRAWS * len(r_last) == len(U)
    case = Case(A, max_tables, batch_recs, U)
    # uploads: the first half in three uneven pieces and a sync ...
    cuts = [0, late_from // 3 + 1, (2 * late_from) // 3 + 5, late_from]
    for a, b in zip(cuts[:-1], cuts[1:]):
        case.upload(a, U[a:b])
    case.sync()
    for s in range(n_submits // 2):
        case.submit(per_submit[s])
    # ... the second half: sentinels (every sample at the top of its range) synced, then the real values, and no sync
    case.upload(late_from, np.full(len(U) - late_from, 1.0 - 2.0**-53))
    case.sync()
    mid = (late_from + len(U)) // 2 + 1
    case.upload(late_from, U[late_from:mid])
    case.upload(mid, U[mid:])
    for s in range(n_submits // 2, n_submits):
        case.submit(per_submit[s])
    case.finish()
    return case


def _order_job(A):
    """A row of weight 1 after ten of weight 1e-16, all samples in one bin: 1000 additions of 1e-16 first make a difference that
    100 additions of 1 first would swallow (the reference's order is the file's)."""
    thr = guards(A)[0]
    b = F32(math.sqrt(thr[A // 2] * thr[A // 2 + 1])) if A > 1 else F32(thr[1] / 2)
    e = np.nextafter(b, F32(np.inf))
    recs = np.zeros(11, REC)
    for i in range(10):
        recs[i] = (b, e, 1e-16, 5e-324)
    recs[10] = (b, e, 1.0, 2.2e-310)
    return recs


def _run_and_check(case, tmp_path):
    r, tables, flags = case.run(tmp_path)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return check(case, tables, flags)


# ---------------------------------------------------------------------------------------------------- the tests
NRECS = (1, 2, 63, 64, 65, 1000, 1200)


def _main_plan(rng):
    counts = (1, 3, 5, 4, 1, 3, 5, 2, 3, 1, 5, 3)  # (12 submits: both staging buffers and all 4 device buffers reused)
    return [[int(NRECS[rng.integers(len(NRECS))]) for _ in range(c)] for c in counts]


def test_fill_kernel_matches_float64_reference_A185(tmp_path):
    """The CLI's grid (A = 185): random F / non-F rows, host-made and stress weights, every hand-placed edge, 12 submits with
    uploads in pieces and a submit that must wait for the uploads it was not synced after."""
    rng = np.random.default_rng(185)
    plan = _main_plan(rng)
    plan[2][0], plan[3][1], plan[7][1] = 1000, 1, 65  # (make sure each length class is there)
    plan[5][0], plan[9][0], plan[11][2] = 63, 64, 2
    order = _order_job(185)
    case = build_case(185, 1, 12, plan, batch_recs=8192, hand_ks=(1, 64, 65, 100, 184, 185), extra_jobs=[order])
    # the fixture is order-sensitive: the order row's table summed in reverse differs in its bits
    t, recs, u_off = case.jobs[-1]
    fwd = expected(recs, u_off, case.U, 185)
    rev = expected(recs, u_off, case.U, 185, order=range(len(recs) - 1, -1, -1))
    assert not fwd[2] and not np.array_equal(fwd[0].view(np.uint64), rev[0].view(np.uint64))
    clean, flagged = _run_and_check(case, tmp_path)
    assert clean >= 30 and flagged >= 10, (clean, flagged)


@pytest.mark.parametrize("A", [1, 64, 65, 256])
def test_fill_kernel_matches_float64_reference_other_grids(A, tmp_path):
    """Grids of 1 bin, exactly one and just over one lane slot, and all four slots: fewer rows, the same edges at the first and
    last steps and at the slot boundary."""
    rng = np.random.default_rng(A)
    plan = [[int(NRECS[rng.integers(5)]) for _ in range(c)] for c in (1, 3, 5, 3)]
    ks = sorted({1, A} | ({64, 65} & set(range(1, A + 1))))
    case = build_case(A, 2, 4, plan, batch_recs=2048, hand_ks=ks, extra_jobs=[_order_job(A)])
    clean, flagged = _run_and_check(case, tmp_path)
    assert clean >= 5 and flagged >= 3, (clean, flagged)


@pytest.mark.parametrize("A", [0, 257])
def test_create_refuses_grids_outside_the_lane_slots(A, tmp_path):
    case = Case(A, 4, 1024, np.zeros(DRAWS + 1))
    case.finish()
    r, _, _ = case.run(tmp_path)
    assert r.returncode == 3, r
    assert b"create failed: age bins outside 1 .. 256" in r.stderr, r.stderr


def test_submit_refuses_more_records_than_a_batch(tmp_path):
    """submit() of more records than batch_recs returns an error and launches nothing: the same DeviceFill still serves the
    next submit; a plain SUBMIT of too many records ends the run with the error."""
    A = 185
    rng = np.random.default_rng(7)
    U = rng.uniform(size=DRAWS * 1100 + 1)
    big = random_recs(rng, 1025, A, wide=False)
    small = random_recs(rng, 40, A, wide=False)
    case = Case(A, 6, 1024, U)
    case.upload(0, U)
    case.submit([(2, big, 1)], refuse=True)
    case.submit([(4, small, 101)])
    case.finish()
    clean, flagged = _run_and_check(case, tmp_path)
    assert (clean, flagged) == (1, 0)
    assert len(case.jobs) == 1  # (table 2 of the refused submit stays +0.0 and unflagged: check() saw no job for it)
    case = Case(A, 6, 1024, U)
    case.upload(0, U)
    case.submit([(2, big, 1)])
    case.finish()
    r, _, _ = case.run(tmp_path, "plain")
    assert r.returncode == 3 and b"submit failed: batch larger than its buffers" in r.stderr, r


def test_f_path_sample_near_float_max_is_dropped_unflagged(tmp_path):
    """F-path rows (begin = 0) up to FLT_MAX and to 1e30: every sample beyond the grid is dropped, unflagged, as on the host --
    also where the kernel's single-precision candidate bin (from 10 x in float) overflows."""
    A = 185
    rng = np.random.default_rng(3)
    U = rng.uniform(size=3 * DRAWS + 1)
    U[1] = 1.0 - 2.0**-53
    recs = np.zeros(1, REC)
    recs[0] = (0.0, FLT_MAX, 0.0, 0.01)
    recs2 = np.zeros(1, REC)
    recs2[0] = (0.0, 1e30, 0.0, 0.01)
    case = Case(A, 3, 1024, U)
    case.upload(0, U)
    case.submit([(0, recs, 1), (2, recs2, 201)])
    case.finish()
    assert _run_and_check(case, tmp_path) == (2, 0)
