"""`Colate --mode CondCoalRates --pairs` on the host twin under AddressSanitizer + UndefinedBehaviorSanitizer (the CPU build
`make -C colate_amd/csrc asan`, device entry points stubbed by tools/no_device_stubs.cpp): one list over a committed
fixture runs clean and writes the tables of the regular build."""
import os
import subprocess

import pytest

import ccpairs_lib as pl
import condcoal_lib as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_CLI = os.path.join(ROOT, "colate_amd", "bin", "Colate_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "colate_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)


def test_pairs_host_twin_clean_under_asan(tmp_path):
    pl.copy_dir(cl.case_dir("boot"), tmp_path)
    shared = ["--mode", "CondCoalRates", "--input", "in", "--poplabels", "in.poplabels", "--lineage_bin", "4",
              "--num_bootstraps", "3", "--seed", "5"]
    pl.write_list(tmp_path / "list.txt", [("PA,PB", "a.txt"), ("PB,PB", "b.txt"), ("PC,PZ", "c.txt")])
    r = subprocess.run([ASAN_CLI] + shared + ["--pairs", "list.txt"], cwd=str(tmp_path), capture_output=True, text=True,
                       env=ENV)
    err = r.stderr
    assert "ERROR: AddressSanitizer" not in err and "runtime error:" not in err and "LeakSanitizer" not in err, err[-3000:]
    assert r.returncode == 0, err[-2000:]
    pl.write_list(tmp_path / "plain.txt", [("PA,PB", "pa.txt"), ("PB,PB", "pb.txt"), ("PC,PZ", "pc.txt")])
    r = pl.run(tmp_path, shared + ["--pairs", "plain.txt"], device=False)
    assert r.returncode == 0, r.stderr[-2000:]
    for a, b in (("a", "pa"), ("b", "pb"), ("c", "pc")):
        assert (tmp_path / f"{a}.txt").read_bytes() == (tmp_path / f"{b}.txt").read_bytes()
