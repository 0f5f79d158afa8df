"""`CoalRate --mode tree` on the host twin under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer
(the CPU builds `make -C colate_amd/csrc asan tsan`, the device walker stubbed by tools/no_device_stubs.cpp): fixtures with
sample ages, several chromosomes and tied times run clean and write the .coal of the regular build."""
import json
import os
import subprocess

import pytest

import coalrate_tree_lib as tl

BIN = os.path.join(tl.ROOT, "colate_amd", "bin")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", TSAN_OPTIONS="exitcode=98")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(tl.ROOT, "colate_amd", "csrc"), "asan", "tsan"], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("exe", ["CoalRate_asan", "CoalRate_tsan"])
@pytest.mark.parametrize("name", ["ancient", "chr", "ties"])
def test_host_twin_clean_under_sanitizers(exe, name, tmp_path):
    d = tl.case_dir(name)
    with open(os.path.join(d, "case.json")) as f:
        args = json.load(f)["args"]
    args[args.index("-o") + 1] = str(tmp_path / "san")
    r = subprocess.run([os.path.join(BIN, exe)] + args, cwd=d, capture_output=True, text=True, env=ENV, timeout=600)
    err = r.stderr
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer", "WARNING: ThreadSanitizer"):
        assert bad not in err, err[-3000:]
    assert r.returncode == 0, err[-2000:]
    r = tl.run_case(name, str(tmp_path / "plain"), device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "san.coal").read_bytes() == (tmp_path / "plain.coal").read_bytes()
