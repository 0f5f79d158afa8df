"""The two CoalRate device paths (coalrate_kernel.hip: cr_count / cr_fold; coalrate_tree_kernel.hip: crt_sort / crt_fold) over
coalrate_edges_lib's case library: every lanes-per-call class, calls that share a workgroup up to the lane cap, both sides
of the LDS boundaries, N = 16384, the largest G and E, and the constructed trees.  Per case the device's sums equal the host
twin's bit for bit, and the launch-shape getters report the shape the case was built for (lanes per call, calls per
workgroup, LDS or device memory, launches) -- a case that took another path fails.  The twin itself is held to the
independent models in test_coalrate_edges_cpu.py.
Every GPU step runs in a child process under a time limit of its own (the twin of all cases of a mode in one child, once);
a test stops at the first child that fails."""
import numpy as np
import pytest

import coalrate_edges_lib as el

pytestmark = pytest.mark.gpu

CHILD_S = 120
ALL = [(mode, name) for mode in ("la", "tree") for name in el.names(mode)]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """mode -> the host twin's num_<case> / den_<case> of every case, computed once in one child per mode."""
    done = {}

    def get(mode):
        if mode not in done:
            try:
                done[mode] = el.run_child(tmp_path_factory.mktemp(f"twin_{mode}"), mode, "all", device=False, timeout=300)
            except Exception as e:      # (a twin child that failed is not run again for the next case)
                done[mode] = e
        if isinstance(done[mode], Exception):
            raise done[mode]
        return done[mode]
    return get


@pytest.mark.parametrize("mode,name", ALL, ids=[f"{mode}-{name}" for mode, name in ALL])
def test_device_equals_host_twin_and_takes_the_expected_path(mode, name, tmp_path, twin):
    c = el.case(mode, name)
    hnum, hden = twin(mode)[f"num_{name}"], twin(mode)[f"den_{name}"]
    out = el.run_child(tmp_path, mode, name, device=True, timeout=CHILD_S)
    got = dict(zip(el.SHAPE_KEYS, (int(v) for v in out["shape"])))
    expect = dict(c["expect"])
    if c["packed"]:
        cus = int(out["cus"])
        calls = int((c["weights"] != 0).sum()) if mode == "la" else len(c["weights"])
        cpw = el.packed_cpw(calls, expect["lanes_per_call"], cus)
        assert got["cpw_min"] == got["cpw_max"] == cpw, (f"{cus} CUs", got, cpw)
        # the case is sized for the lane cap on a 256-CU chip: on another chip it must say so, not test less
        assert cpw == expect["cpw_max"] and cpw * expect["lanes_per_call"] == el.K_MAX_LANES, (f"{cus} CUs", got, expect)
    assert got == expect, (got, expect)
    assert (hnum != 0).any() and (name.startswith("all_at_zero") or (hden != 0).any())
    assert el.same_bits(out["num"], hnum)
    assert el.same_bits(out["den"], hden)


def test_refusals_leave_the_device_usable(tmp_path):
    """G = 320 at N = 8 and E = 1025 are refused with COLATE_ELIMIT and a message that says why, without a launch; the nearest
    accepted input then runs in the same process, on its expected path, with the twin's bits."""
    out = el.run_child(tmp_path, "refusals", "-", device=True, timeout=CHILD_S)
    assert int(out["la_code"]) == -4 and "do not fit the LDS" in str(out["la_message"]), out["la_message"]
    assert int(out["tree_code"]) == -4 and "more than the kernel keeps in LDS (1024)" in str(out["tree_message"]), out["tree_message"]
    assert "1025 epochs" in str(out["tree_message"])
    for mode, ok in (("la", "max_G"), ("tree", "E_1024")):
        assert not out[f"{mode}_shape_refused"].any()
        assert dict(zip(el.SHAPE_KEYS, out[f"{mode}_shape"].tolist())) == el.case(mode, ok)["expect"]
        assert bool(out[f"{mode}_same"])
