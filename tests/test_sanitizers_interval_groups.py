"""The host side of colate_interval_fit_groups and of the many-pairs record collection under AddressSanitizer +
UndefinedBehaviorSanitizer: the stand-alone program csrc/tools/interval_groups_check.cpp (its own main; `make -C colate_amd/csrc
asan` builds it with g++ -fsanitize=address,undefined and the device entry points stubbed by tools/no_device_stubs.cpp) runs the
host twin against the two host calls group by group, the refusals, and collect_interval_records_pairs against the single-pair
walk over inputs it writes into a scratch directory, and ends clean."""
import os
import subprocess

import interval_cells_lib as il

BIN = os.path.join(il.ROOT, "colate_amd", "bin")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_host_twin_checks_and_record_collection_clean_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(il.ROOT, "colate_amd", "csrc"), "../bin/interval_groups_check_asan"],
                          stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(BIN, "interval_groups_check_asan"), str(tmp_path)], capture_output=True, text=True, env=ENV, timeout=300)
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert bad not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.stdout[-1000:], r.stderr[-2000:])
