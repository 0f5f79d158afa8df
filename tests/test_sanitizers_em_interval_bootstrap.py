"""The host side of colate_bootstrap_em_interval_batch under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
program csrc/tools/em_interval_bootstrap_check.cpp (its own main; `make -C colate_amd/csrc asan` builds it with g++
-fsanitize=address,undefined and the device entry points stubbed by tools/no_device_stubs.cpp) runs the rows-file parser
on good and malformed files, colate_bootstrap_rows_host and both host twins of the fit, and ends clean."""
import os
import subprocess

import em_interval_bootstrap_lib as bl

BIN = os.path.join(bl.ROOT, "colate_amd", "bin")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_host_twins_and_parser_clean_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(bl.ROOT, "colate_amd", "csrc"), "../bin/em_interval_bootstrap_check_asan"],
                          stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(BIN, "em_interval_bootstrap_check_asan"), str(tmp_path)], capture_output=True, text=True, env=ENV,
                       timeout=300)
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.stdout[-1000:], r.stderr[-2000:])
