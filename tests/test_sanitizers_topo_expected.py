"""The host forms of `Colate --mode count_topo --expected` under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
program csrc/tools/topo_expected_check.cpp (its own main; built with g++ -fsanitize=address,undefined and the device entry points
stubbed by tools/no_device_stubs.cpp) writes small inputs into a scratch directory, loads and indexes them through the loader of the
command line, compares the cursor path -- the walk's sink forming the fixed-point addends -- with colate_topo_expected_blocks_host
for every triple -- for 1, the command line's and 1024 epochs and three block sizes --, repeats the walk on counts beyond 16 bits,
checks the addends against a 128-bit quotient, runs the refusals, and ends clean.  Nothing sanitized is loaded into Python."""
import os
import subprocess

import interval_cells_lib as il

BIN = os.path.join(il.ROOT, "colate_amd", "bin")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
for _k in ("COLATE_DEVICE_TOPO", "COLATE_INDEXED_WALK"):
    ENV.pop(_k, None)


def test_cursor_path_equals_the_twin_and_the_addends_run_clean_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(il.ROOT, "colate_amd", "csrc"), "../bin/topo_expected_check_asan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(BIN, "topo_expected_check_asan"), str(tmp_path)], capture_output=True, text=True, env=ENV, timeout=300)
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.stdout[-1000:], r.stderr[-2000:])
