"""What `Colate` says and writes on the device, with nothing set: the seven list-mode lines and the four single runs of
cli_transcripts_lib to the end, against the device transcripts of tests/golden/cli_transcripts, and every file that the host run of
the same line writes too, byte for byte.  (The host runs of the three `mut` lines stop at their .counts files, which the device runs
do not write: of these lines the transcript alone is compared.)"""
import shutil

import pytest

import cli_transcripts_lib as ct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    return ct.stage(tmp_path_factory.mktemp("transcripts") / "in")


@pytest.mark.parametrize("line", ct.DEVICE_LINES, ids=lambda l: l.name)
def test_device_run_says_and_writes_what_it_did(staged, tmp_path, line):
    inputs = set(ct.files_of(staged))
    for sub in ("host", "device"):
        shutil.copytree(staged, tmp_path / sub)
    code, said = ct.run_line(ct.CLI, tmp_path / "device", line, host=False)
    assert said == ct.golden(line.name, "device")
    assert code == 0
    assert ct.run_line(ct.CLI, tmp_path / "host", line, host=True)[0] == 0
    host, device = ct.files_of(tmp_path / "host"), ct.files_of(tmp_path / "device")
    assert set(device) - inputs, "the device run wrote no file"
    for name in sorted(set(host) - inputs):
        if name in device:  # (`--counts_only` stops the host run of a `mut` line at its .counts files: these the device run does not write)
            assert host[name] == device[name], name
        else:
            assert name.endswith(".counts"), name
