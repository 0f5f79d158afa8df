"""The host side of the interval cells under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone program
csrc/tools/interval_cells_check.cpp (its own main; `make -C colate_amd/csrc asan` builds it with g++
-fsanitize=address,undefined and the device entry points stubbed by tools/no_device_stubs.cpp) runs the threshold builder
and colate_interval_cells_host against a plain ordered loop, the refusals included, and ends clean."""
import os
import subprocess

import interval_cells_lib as il

BIN = os.path.join(il.ROOT, "colate_amd", "bin")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_threshold_builder_and_host_twin_clean_under_sanitizers():
    subprocess.check_call(["make", "-C", os.path.join(il.ROOT, "colate_amd", "csrc"), "../bin/interval_cells_check_asan"],
                          stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(BIN, "interval_cells_check_asan")], capture_output=True, text=True, env=ENV, timeout=300)
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.stdout[-1000:], r.stderr[-2000:])
