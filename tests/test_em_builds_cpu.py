"""The dispatch of the EM kernel (csrc/em_build.hpp) at every boundary, without a device: colate_em_kernel_build_for answers from
given numbers -- batch size, epoch count, compute units, forced variant -- and the launch switches on the same table entry.

The expected names are written out below, per epoch count and per region of the batch size:
  alone    B <= #CUs             every workgroup has a CU to itself
  shared   #CUs < B <= 2 #CUs    two workgroups on a CU
  beyond   B > 2 #CUs
A device whose CU count could not be asked (cus = 0) is treated as `shared` at every batch size."""
import ctypes

import pytest

E_VALUES = (2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
CUS = (32, 256, 304)

# chunks x rows of the instantiations for E <= 128
SHAPE = {2: "1x1", 16: "1x1", 17: "1x2", 32: "1x2", 33: "1x4", 64: "1x4", 65: "2x4", 128: "2x4"}
# beyond 128 epochs nothing is chosen: B, the CU count and the forced variant do not matter
FIXED = {129: "default-tput/4x4", 256: "default-tput/4x4", 257: "big-tput/8x4", 512: "big-tput/8x4", 513: "big-tput/16x4",
         1024: "big-tput/16x4"}
ESTEP = {2: "default-estep/1x4", 16: "default-estep/1x4", 17: "default-estep/1x4", 32: "default-estep/1x4", 33: "default-estep/1x4",
         64: "default-estep/1x4", 65: "default-estep/2x4", 128: "default-estep/2x4", 129: "default-estep/4x4", 256: "default-estep/4x4",
         257: "big-estep/8x4", 512: "big-estep/8x4", 513: "big-estep/16x4", 1024: "big-estep/16x4"}
# (forced variant, region) -> unit and kind for 1 epoch per lane (E <= 64) ...
KIND_1 = {
    (None, "alone"): "ilp-free", (None, "shared"): "ilp-capped", (None, "beyond"): "default-tput",
    ("latency-ilp", "alone"): "ilp-free", ("latency-ilp", "shared"): "ilp-capped", ("latency-ilp", "beyond"): "ilp-capped",
    ("latency", "alone"): "default-capped", ("latency", "shared"): "default-capped", ("latency", "beyond"): "default-capped",
    ("throughput", "alone"): "default-tput", ("throughput", "shared"): "default-tput", ("throughput", "beyond"): "default-tput",
}
# ... and for 2 (65 <= E <= 128): there is no free build
KIND_2 = dict(KIND_1)
KIND_2[(None, "alone")] = KIND_2[("latency-ilp", "alone")] = "ilp-capped"

FORCED = (None, "latency-ilp", "latency", "throughput")


def expected(B_region, E, forced):
    if E > 128:
        return FIXED[E]
    return (KIND_1 if E <= 64 else KIND_2)[(forced, B_region)] + "/" + SHAPE[E]


def batches(cus):
    """(B, region) on both sides of each boundary."""
    if cus == 0:
        return [(1, "shared"), (2, "shared"), (513, "shared"), (100000, "shared")]
    return [(1, "alone"), (cus, "alone"), (cus + 1, "shared"), (2 * cus, "shared"), (2 * cus + 1, "beyond")]


@pytest.fixture(scope="module")
def ca():
    import colate_amd

    return colate_amd


@pytest.mark.parametrize("cus", CUS + (0,))
def test_em_fit_dispatch_at_every_boundary(ca, cus):
    for B, region in batches(cus):
        for E in E_VALUES:
            for forced in FORCED:
                assert ca.em_kernel_build_for(B, E, cus, forced) == expected(region, E, forced), (B, E, cus, forced)


def test_estep_dispatch_ignores_batch_and_forcing(ca):
    for cus in CUS + (0,):
        for B, _ in batches(cus):
            for E in E_VALUES:
                for forced in FORCED:
                    assert ca.em_kernel_build_for(B, E, cus, forced, mode=1) == ESTEP[E], (B, E, cus, forced)


def test_the_names_reached_are_the_names_listed(ca):
    """colate_em_kernel_builds is generated from the table the dispatch looks its answer up in: what the boundaries above reach, over
    all CU counts and forced values, is exactly that list -- no build that nothing selects, none that has no name."""
    reached = {0: set(), 1: set()}
    for cus in CUS + (0,):
        for B, _ in batches(cus):
            for E in E_VALUES:
                for forced in FORCED:
                    for mode in (0, 1):
                        reached[mode].add(ca.em_kernel_build_for(B, E, cus, forced, mode=mode))
    for mode in (0, 1):
        listed = ca.em_kernel_builds(mode)
        assert len(listed) == len(set(listed))
        assert reached[mode] == set(listed), (mode, sorted(reached[mode] ^ set(listed)))
    assert len(ca.em_kernel_builds(0)) == 18 and len(ca.em_kernel_builds(1)) == 5
    # the written-out tables name the same sets
    want0 = {k + "/" + s for k in set(KIND_1.values()) for s in ("1x1", "1x2", "1x4")} | {k + "/2x4" for k in set(KIND_2.values())}
    assert set(ca.em_kernel_builds(0)) == want0 | set(FIXED.values())
    assert set(ca.em_kernel_builds(1)) == set(ESTEP.values())


def test_variant_of_a_name(ca):
    """colate_em_kernel_variant keeps its three values; they are a function of the build: unit ilp = "latency-ilp", a capped build
    of the default unit = "latency", every two-wave build = "throughput"."""
    assert ca.api.EM_VARIANTS == ("latency-ilp", "latency", "throughput")
    for forced in FORCED[1:]:
        for E in (2, 23, 64, 65, 128):
            for B in (1, 300, 600):
                name = ca.em_kernel_build_for(B, E, 256, forced)
                assert name.startswith({"latency-ilp": "ilp-", "latency": "default-capped/", "throughput": "default-tput/"}[forced])


def test_refusals(ca):
    name = ctypes.create_string_buffer(64)
    lib = ca.api.lib
    assert lib.colate_em_kernel_build_for(0, 4, 0, 256, -1, name, 64) < 0      # E < 1
    assert lib.colate_em_kernel_build_for(0, 4, 1025, 256, -1, name, 64) < 0   # E beyond the compiled limit
    assert lib.colate_em_kernel_build_for(2, 4, 23, 256, -1, name, 64) < 0     # no such mode
    assert lib.colate_em_kernel_build_for(0, -1, 23, 256, -1, name, 64) < 0
    assert lib.colate_em_kernel_build_for(0, 4, 23, 256, -1, name, 12) < 0     # "ilp-free/1x2" needs 13 bytes
    assert lib.colate_em_kernel_build_for(0, 4, 23, 256, -1, name, 13) == 12 and name.value == b"ilp-free/1x2"
    assert lib.colate_em_kernel_build_for(0, 4, 23, 256, 7, name, 64) == 12    # a forced value out of range = automatic
    buf = ctypes.create_string_buffer(2048)
    n = lib.colate_em_kernel_builds(0, buf, 2048)
    assert n == len(buf.value) > 0
    assert lib.colate_em_kernel_builds(0, buf, n) < 0 and lib.colate_em_kernel_builds(0, buf, n + 1) == n
    assert lib.colate_em_kernel_builds(3, buf, 2048) == 0 and buf.value == b""  # a mode without builds: the empty list
