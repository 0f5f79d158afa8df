"""The case library of the CoalRate edge tests on the CPU (coalrate_edges_lib.py; no GPU needed): every case's self-check
(the case is what its name says and is sized for the launch shape it expects), and the host twin against the independent
models -- the pair-by-pair restatement (coalrate_model.Model, bound check_against), the exact integer model (la_exact: equal
bits), the numpy restatement of coal_tree::populate (coalrate_tree_model.accumulate, bound within_bound) and the sums
written out by hand.  Tiled cases check their distinct trees once.  The GPU test (test_gpu_coalrate_edges.py) then holds the
device to the twin bit for bit."""
import numpy as np
import pytest

import coalrate_edges_lib as el
import coalrate_model as cm
import coalrate_tree_model as tm
import colate_amd

ALL = [(mode, name) for mode in ("la", "tree") for name in el.names(mode)]
IDS = [f"{mode}-{name}" for mode, name in ALL]


def test_the_library_holds_every_case():
    la, tree = set(el.names("la")), set(el.names("tree"))
    assert {f"lpc_{k}" for k in (1, 4, 8, 16, 32, 64, 128, 256)} <= la
    assert {"packed_two_waves", "packed_cap", "lds_last", "lds_first", "max_N_G1", "max_N_G2", "max_G", "empty_group", "one_group",
            "returning_blocks", "all_zero_weight_chunk", "smallest", "all_in_last_epoch"} <= la
    assert {f"lpc_{N}" for N in (2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)} <= tree
    assert {"packed_two_waves", "packed_cap", "max_N", "E_2", "E_1024"} <= tree
    assert {f"{n}_{N}" for n in el.TREE_SHAPED for N in (40, 300)} <= tree
    assert {el.case("la", f"lpc_{k}")["expect"]["lanes_per_call"] for k in el.G_OF_LPC} == {1, 4, 8, 16, 32, 64, 128, 256}
    assert {el.case("tree", f"lpc_{N}")["expect"]["lanes_per_call"] for N in el.TREE_LPC_N} == {4, 8, 16, 32, 64, 128, 256}


@pytest.mark.parametrize("mode,name", ALL, ids=IDS)
def test_self_check(mode, name):
    c = el.case(mode, name)
    c["check"](c)
    T, nn = c["parents"].shape
    N = (nn + 1) // 2
    x = c["expect"]
    assert set(x) == set(el.SHAPE_KEYS)
    if mode == "la":
        assert x["lanes_per_call"] == el.la_lpc(c["G"]) and x["lds"] == (sum(el.la_lds_bytes(N, c["G"])) <= el.K_LDS_BYTES)
        assert el.la_lds_bytes(N, c["G"])[0] <= el.K_LDS_BYTES and c["groups"].max() < c["G"] and c["groups"].shape[1] == N
        calls = [int((c["weights"][i:i + (c["chunk"] or T)] != 0).sum()) for i in range(0, T, c["chunk"] or T)]
    else:
        assert x["lanes_per_call"] == el.tree_lpc(N) and x["lds"] == (el.tl.padded_keys(N) <= el.K_LDS_KEYS)
        assert len(c["epochs"]) <= el.K_MAX_EPOCHS
        calls = [len(c["weights"][i:i + (c["chunk"] or T)]) for i in range(0, T, c["chunk"] or T)]
    assert x["launches"] == sum(1 for n in calls if n)          # one first-kernel launch per chunk that holds a call
    if not c["packed"]:                                         # fewer calls than any chip has wave slots: never packed
        assert x["cpw_min"] == x["cpw_max"] == 1 and max(calls) * ((x["lanes_per_call"] + 63) // 64) <= 64 * el.K_WAVES_PER_CU
    assert len(c["weights"]) == len(c["blocks"]) == T and c["blocks"].max() < c["num_blocks"]
    assert c["distinct"] is None or (T % c["distinct"] == 0 and el.same_bits(
        c["bl"], np.tile(c["bl"][:c["distinct"]], (T // c["distinct"], 1))))


def test_the_refused_inputs_are_one_step_beyond_the_accepted():
    r = el.refused_cases()
    assert r["la"]["G"] == el.case("la", "max_G")["G"] + 1 == 320 and r["la"]["parents"].shape[1] == 15
    assert len(r["tree"]["epochs"]) == len(el.case("tree", "E_1024")["epochs"]) + 1 == 1025
    # both are valid inputs: the host twin takes them
    for c in r.values():
        num, den = el.accumulate(c, False)
        assert (num != 0).any() and (den != 0).any()


def _pairwise(c, first):
    model = cm.Model(c["epochs"], c["num_blocks"], c["G"])
    for k in range(first):
        if c["weights"][k] != 0.0:      # (a tree of weight 0 makes no call; the model would add zeros)
            model.populate(c["parents"][k], c["bl"][k], float(c["weights"][k]), c["groups"][c["gv"][k]], int(c["blocks"][k]), c["ages"])
    return model


@pytest.mark.parametrize("mode,name", ALL, ids=IDS)
def test_host_twin_against_the_models(mode, name):
    c = el.case(mode, name)
    first = c["distinct"] or len(c["weights"])
    N = (c["parents"].shape[1] + 1) // 2
    num, den = el.accumulate(c, False, first=first)
    assert (num != 0).any() and (name.startswith("all_at_zero") or (den != 0).any())      # (the GPU test compares more than zeros)
    checked = []
    if c["hand"] is not None:
        assert el.same_bits(num, c["hand"][0]) and el.same_bits(den, c["hand"][1])
        checked.append("hand")
    if c["model"] == "exact":
        enum, eden = el.la_exact(c)
        assert (enum != 0).any() and (eden != 0).any()
        assert el.same_bits(num, enum) and el.same_bits(den, eden)
        checked.append("exact")
    if mode == "la" and (c["model"] == "pairwise" or N <= 300 and c["G"] <= 3):
        assert N <= 300 and first <= 50
        worst = cm.check_against(_pairwise(c, first), num, den)
        checked.append(f"pairwise (largest |difference| / bound = {worst:.3g})")
    if mode == "tree":
        mnum, mden, n_num, n_den = tm.accumulate(c["parents"][:first], c["bl"][:first], c["weights"][:first], c["blocks"][:first],
                                                 c["num_blocks"], c["epochs"], c["ages"])
        assert (mnum != 0).any()
        assert ((num == 0) == (mnum == 0)).all() and ((den == 0) == (mden == 0)).all()
        assert tm.within_bound(num, mnum, n_num) and tm.within_bound(den, mden, n_den)
        checked.append("tree model")
    assert checked
    print(f"{mode} {name}: {', '.join(checked)}")


def test_exact_model_cases_are_also_within_the_pairwise_bound():
    """la_exact itself is held to the literal model where that is affordable (N = 8)."""
    for name in ("empty_group", "one_group"):
        c = el.case("la", name)
        enum, eden = el.la_exact(c)
        cm.check_against(_pairwise(c, len(c["weights"])), enum, eden)


def test_caterpillar_of_16384_leaves_in_one_group_closed_form():
    """The node at time q joins one leaf to q leaves: q * 1 pairs.  num[e] = the sum of q over the cell; denom[e] = the later
    pairs times the cell's width plus the sum of q (q - epochs[e]) over the cell."""
    c = el.case("la", "max_N_G1")
    num, den = el.accumulate(c, False, first=1)
    assert c["weights"][0] == 1e9 and c["blocks"][0] == 0
    q = np.arange(1, el.K_MAX_N, dtype=np.int64)
    ep = c["epochs"].astype(np.int64)
    for e in range(len(ep) - 1):
        cell, later = (q > ep[e]) & (q <= ep[e + 1]), q > ep[e + 1]
        assert num[0, 0, 0, e] == q[cell].sum()
        assert den[0, 0, 0, e] == (ep[e + 1] - ep[e]) * q[later].sum() + (q[cell] * (q[cell] - ep[e])).sum()
    assert num[0, 0, 0].sum() == el.K_MAX_N * (el.K_MAX_N - 1) // 2 and not num[1].any()


def test_constructed_group_vectors_leave_the_right_cells_empty():
    c = el.case("la", "empty_group")
    num, den = el.accumulate(c, False)
    assert not num[:, 1].any() and not num[:, :, 1].any() and not den[:, 1].any() and not den[:, :, 1].any()
    assert num[:, 2, 0].any() and num[:, 0, 0].any() and num[:, 2, 2].any()
    c = el.case("la", "one_group")
    num, den = el.accumulate(c, False)
    only = np.zeros(num.shape, dtype=bool)
    only[:, 0, 0] = only[:, 2, 2] = True
    assert not num[~only].any() and not den[~only].any() and num[:, 0, 0].any() and num[:, 2, 2].any()
    N = c["parents"].shape[1] // 2 + 1
    assert num[:, 2, 2].sum() + num[:, 0, 0].sum() == N * (N - 1) // 2 * (c["weights"] / 1e9).sum()     # every pair meets once


@pytest.mark.parametrize("mode,name", [("la", "returning_blocks"), ("tree", "returning_blocks_40"), ("tree", "returning_blocks_300")])
def test_returning_blocks_equal_the_calls_sorted_by_block(mode, name):
    """A stable sort by block keeps every block's calls in their order, so its sums keep their bits."""
    c = el.case(mode, name)
    num, den = el.accumulate(c, False)
    order = np.argsort(c["blocks"], kind="stable")
    s = dict(c)
    for key in ("parents", "bl", "weights", "blocks") + (("gv",) if mode == "la" else ()):
        s[key] = c[key][order]
    assert (np.diff(s["blocks"]) >= 0).all() and (order != np.arange(len(order))).any()
    snum, sden = el.accumulate(s, False)
    assert el.same_bits(num, snum) and el.same_bits(den, sden) and all(num[b].any() for b in range(c["num_blocks"]))


def test_a_chunk_of_weight_zero_adds_nothing():
    c = el.case("la", "all_zero_weight_chunk")
    num, den = el.accumulate(c, False)
    fnum, fden = el.accumulate(c, False, first=4)
    assert el.same_bits(num, fnum) and el.same_bits(den, fden) and num.any()


def test_launch_shape_getters_report_nothing_without_a_device_call():
    el.accumulate(el.case("la", "smallest"), False)
    el.accumulate(el.case("tree", "E_2"), False)
    for got in (colate_amd.coalrate_launch_shape(), colate_amd.coalrate_tree_launch_shape()):
        assert tuple(got) == el.SHAPE_KEYS and not any(got.values())
