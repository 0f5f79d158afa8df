"""colate_interval_fit_groups_host and `Colate --mode mut_interval --pairs` without a device: the host twin of the grouped
call equals, bit for bit, the composition of the two host calls it stands for, and every OUTPUT.coal of a --pairs run is the
file of its single run, byte for byte."""
import numpy as np
import pytest

import colate_amd
import interval_cells_lib as il
import interval_groups_lib as gl

B = 3


def _cases():
    four = gl.four_groups(B)
    return {
        "G1": [gl.with_weights(il.random_records(80, 2, 31), B, 5)],
        "G4_nb_1_3_5_2": four,
        "no_records_in_the_middle": four[:2] + [gl.with_weights(gl.no_records(2), B, 6)] + four[2:],
        "all_beyond_the_grid": four[:1] + [gl.with_weights(gl.all_beyond(7, 2), B, 7)] + four[3:],
    }


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", ["G1", "G4_nb_1_3_5_2", "no_records_in_the_middle", "all_beyond_the_grid"])
def test_host_twin_equals_the_two_host_calls_per_group(name, math):
    groups = _cases()[name]
    ep = gl.epochs23()
    got = colate_amd.interval_fit_groups(groups, ep, device=False, math=math, **gl.FIT)
    gl.assert_same(got, gl.composed(groups, ep, device=False, math=math, **gl.FIT))
    R, dropped, rates, iters, ll, flags = got
    if name == "G4_nb_1_3_5_2":
        assert [g[5] for g in groups] == [1, 3, 5, 2] and (R > 0).all() and (iters >= 10).all()
    if name == "no_records_in_the_middle":
        assert R[2] == 0 and dropped[2] == 0
    if name == "all_beyond_the_grid":
        assert R[1] == 0 and dropped[1] == 7
    for g in np.flatnonzero(R == 0):
        assert (rates[g] == colate_amd.DEFAULT_INIT_RATE).all() and not iters[g].any() and not ll[g].any() and not flags[g].any()


def test_per_group_epochs_and_starting_rates():
    groups = gl.four_groups(B)[:2]
    ep = np.stack([gl.epochs23(), gl.epochs23() * 1.5])
    init = np.stack([np.full(ep.shape[1], 1e-4), np.full(ep.shape[1], 3e-5)])
    got = colate_amd.interval_fit_groups(groups, ep, init_rates=init, device=False, **gl.FIT)
    for g in range(2):
        one = colate_amd.interval_fit_groups(groups[g:g + 1], ep[g], init_rates=init[g], device=False, **gl.FIT)
        for x, y in zip(got, one):
            assert il.same_bits(x[g:g + 1], y)


def _refused(groups, ep, msg, code=-1, device=False, **kw):
    with pytest.raises(colate_amd.ColateError) as e:
        colate_amd.interval_fit_groups(groups, ep, device=device, **dict(gl.FIT, **kw))
    assert e.value.code == code and msg in str(e.value), str(e.value)


@pytest.mark.parametrize("device", [False, True])
def test_refusals_name_the_group(device):
    """(the device form refuses the same things before it asks for a device)"""
    four, ep = gl.four_groups(B), gl.epochs23()
    b, e, w_sh, w_ns, blk, nb, bw = four[2]
    bad_age = (e, b, w_sh, w_ns, blk, nb, bw)  # begin > end
    _refused(four[:2] + [bad_age], ep, "group 2: record", device=device)
    _refused(four[:1] + [(b, e, w_sh, w_ns, blk[::-1].copy(), nb, bw)], ep, "group 1: record", device=device)
    _refused(four[:1] + [(b, e, w_sh, w_ns, blk, nb, -bw)], ep, "group 1: block weight", device=device)
    _refused(four[:1] + [(b, e, w_sh, w_ns, blk, 4097, np.ones((B, 4097)))], ep, "group 1: nb=4097", code=-4, device=device)
    bad_ep = np.stack([ep, ep[::-1]])
    _refused(four[:2], bad_ep, "group 1: epochs must be non-decreasing", device=device)
    _refused(four[:2], ep + 50.0, "group 0: call 0: age_begin", device=device)  # rows start before epochs[0]
    _refused(four[:2], ep, "max_iter", max_iter=0, device=device)
    _refused([], ep, "bad sizes G=0", device=device)


def test_decreasing_rec_off_is_refused_and_outputs_stay():
    (b, e, w_sh, w_ns, blk, nb, bw), ep = gl.four_groups(B)[0], gl.epochs23()
    recs = np.zeros(b.size, dtype=colate_amd.api.INTERVAL_REC)
    recs["begin"], recs["end"], recs["w_sh"], recs["w_ns"] = b, e, w_sh, w_ns
    rec_off = np.array([0, b.size, b.size - 1], dtype=np.int64)
    nbs, bws = np.array([nb, nb], dtype=np.int32), np.concatenate([bw.ravel(), bw.ravel()])
    E = ep.size
    eps, init = np.tile(ep, 2), np.full(2 * E, 1e-4)
    R, dropped = np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int64)
    rates, iters, ll, flags = np.full((2, B, E), -7.0), np.full((2, B), -7, dtype=np.int32), np.full((2, B), -7.0), np.full((2, B), -7, dtype=np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    rc = colate_amd.api.lib.colate_interval_fit_groups_host(2, B, E, p(rec_off), p(recs), p(blk), p(nbs), p(bws), p(eps), p(init), 40, 10, 1e-3,
                                                            1e-10, p(R), p(dropped), p(rates), p(iters), p(ll), p(flags), 1)
    assert rc == -1 and b"rec_off decreases" in colate_amd.api.lib.colate_last_error()
    assert (R == -7).all() and (dropped == -7).all() and (rates == -7).all() and (iters == -7).all() and (ll == -7).all() and (flags == -7).all()


# ------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def six(tmp_path_factory):
    """the six-line list run on the host, and the single run of each line"""
    d = tmp_path_factory.mktemp("interval_pairs")
    gl.cli_inputs(d)
    gl.write_list(d / "pairs.txt", gl.SIX_PAIRS)
    r = gl.run_pairs(d, "pairs.txt", device=False)
    singles = [gl.run_single(d, pair, "single_" + pair[2], device=False) for pair in gl.SIX_PAIRS]
    return d, r, singles


def test_cli_pairs_coal_files_are_the_single_runs(six):
    d, r, singles = six
    assert r.returncode == 0, r.stderr[-3000:]
    assert "on the host (COLATE_DEVICE_INTERVAL=0)" in r.stderr
    for pair, s in zip(gl.SIX_PAIRS, singles):
        assert s.returncode == 0, s.stderr[-2000:]
        assert (d / (pair[2] + ".coal")).read_bytes() == (d / ("single_" + pair[2] + ".coal")).read_bytes(), pair[2]
    coal = [(d / (pair[2] + ".coal")).read_bytes() for pair in gl.SIX_PAIRS]
    assert coal[0] == coal[4] and coal[0] != coal[1] and coal[0] != coal[2]  # the repeated pair; another target; the mask
    assert len(coal[3].split(b"\n")[1].split()) != len(coal[0].split(b"\n")[1].split())  # another number of epochs


def test_cli_pairs_stderr_lines_are_the_single_runs(six):
    d, r, singles = six
    P = len(gl.SIX_PAIRS)
    for i, s in enumerate(singles):
        lines = gl.pair_lines(r.stderr, i + 1, P)
        assert lines == gl.single_lines(s.stderr) and len(lines) == 3 + 4, (i, lines)
    # more rows than the 512 the fit keeps in registers
    assert il.stderr_count(singles[0], "Number of rows") > 512 and il.stderr_count(singles[1], "Number of rows") > 512
    assert il.stderr_count(singles[0], "Number of blocks") == 8


def test_cli_pairs_one_block(tmp_path):
    gl.cli_inputs(tmp_path, chroms=("1",), snps_per_chr=300, span=20_000_000)
    pairs = gl.SIX_PAIRS[:2]
    gl.write_list(tmp_path / "pairs.txt", pairs)
    r = gl.run_pairs(tmp_path, "pairs.txt", device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    for i, pair in enumerate(pairs):
        s = gl.run_single(tmp_path, pair, "s_" + pair[2], device=False)
        assert s.returncode == 0 and il.stderr_count(s, "Number of blocks") == 1
        assert gl.pair_lines(r.stderr, i + 1, 2) == gl.single_lines(s.stderr)
        assert (tmp_path / (pair[2] + ".coal")).read_bytes() == (tmp_path / ("s_" + pair[2] + ".coal")).read_bytes()


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("interval_pairs_small")
    gl.cli_inputs(d, chroms=("1",), snps_per_chr=300, span=20_000_000)
    return d


@pytest.mark.parametrize("line,msg", [
    ("T.colate.in R.colate.in a 7000", "bad.txt, line 2: --mode mut_interval takes modern samples only"),
    ("T.colate.in R.colate.in a 0", "bad.txt, line 2: --mode mut_interval takes modern samples only"),
    ("T.colate.in R.colate.in a mask=tm", "bad.txt, line 2: unknown key 'mask'"),
])
def test_cli_pairs_bad_lines_are_named(small, line, msg):
    with open(small / "bad.txt", "w") as f:
        f.write("T.colate.in R.colate.in first\n" + line + "\n")
    r = gl.run_pairs(small, "bad.txt", device=False)
    assert r.returncode == 1 and msg in r.stderr, r.stderr[-800:]
    assert not (small / "first.coal").exists()


@pytest.mark.parametrize("option", ["target_tmp", "reference_tmp", "rows", "write_rows", "output", "target_mask", "reference_mask",
                                    "coal", "ranks", "target_age", "reference_age"])
def test_cli_pairs_refused_options_are_named(small, option):
    gl.write_list(small / "ok.txt", gl.SIX_PAIRS[:1], prefix="refused_")
    r = gl.run_pairs(small, "ok.txt", device=False, more=["--" + option, "2"])
    assert r.returncode == 1 and ("--" + option + " cannot be combined with") in r.stderr, r.stderr[-800:]
    assert not (small / "refused_p1.coal").exists()


def test_cli_pairs_need_bins_where_a_line_has_no_coal(small):
    gl.write_list(small / "two.txt", [gl.SIX_PAIRS[3], gl.SIX_PAIRS[0]], prefix="nobins_")
    r = gl.run_pairs(small, "two.txt", device=False, common=["--mut", "P", "--chr", "chr.txt"])
    assert r.returncode == 1 and "--pairs needs --bins for pair 2 (it names no coal= file)." in r.stderr, r.stderr[-800:]


def test_cli_pair_with_an_empty_target_is_named_and_the_others_are_written(small):
    open(small / "empty.colate.in", "wb").close()
    pairs = [gl.SIX_PAIRS[0], ("empty.colate.in", "R.colate.in", "p_empty", [], []), gl.SIX_PAIRS[1]]
    gl.write_list(small / "with_empty.txt", pairs, prefix="e_")
    r = gl.run_pairs(small, "with_empty.txt", device=False)
    assert r.returncode == 1, r.stderr[-1500:]
    assert "Error: pair 2 (empty.colate.in x R.colate.in) uses no SNP within the age grid" in r.stderr
    assert (small / "e_p1.coal").exists() and (small / "e_p2.coal").exists() and not (small / "e_p_empty.coal").exists()
    s = gl.run_single(small, gl.SIX_PAIRS[1], "e_single", device=False)
    assert (small / "e_p2.coal").read_bytes() == (small / "e_single.coal").read_bytes()


def test_cli_pairs_without_seed_share_one_seed(small):
    gl.write_list(small / "twice.txt", [gl.SIX_PAIRS[0], gl.SIX_PAIRS[4]], prefix="ns_")
    r = gl.run_pairs(small, "twice.txt", device=False, fit=["--num_bootstraps", "4", "--max_iter", "60", "--min_iter", "20"])
    assert r.returncode == 0, r.stderr[-1500:]
    assert (small / "ns_p1.coal").read_bytes() == (small / "ns_p5.coal").read_bytes()
