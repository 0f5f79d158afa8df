"""What `Colate` says on the host paths, line for line: every list mode, single run, cursor fallback and refusal of
cli_transcripts_lib against the transcripts of tests/golden/cli_transcripts (recorded before the drivers shared one list front end
and one per-pair back end).  `--counts_only` keeps the `mut` lines off the device, COLATE_DEVICE_*=0 the others."""
import shutil

import pytest

import cli_transcripts_lib as ct


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    return ct.stage(tmp_path_factory.mktemp("transcripts") / "in")


@pytest.mark.parametrize("line", ct.HOST_LINES, ids=lambda l: l.name)
def test_host_run_says_what_it_said(staged, tmp_path, line):
    shutil.copytree(staged, tmp_path / "run")  # (two lines of one directory share output names)
    code, said = ct.run_line(ct.CLI, tmp_path / "run", line, host=True)
    assert said == ct.golden(line.name, "host")
    assert code == 0


@pytest.mark.parametrize("line", ct.UNWRITABLE, ids=lambda l: l.name)
def test_unwritable_pair_file_says_what_it_said(staged, tmp_path, line):
    shutil.copytree(staged, tmp_path / "run")
    code, said = ct.run_line(ct.CLI, tmp_path / "run", line, host=True)
    assert said == ct.golden(line.name, "host")
    assert code == 1 and said.count("cannot write") == 1


@pytest.mark.parametrize("mode", sorted(ct.REFUSALS))
def test_refusals_say_what_they_said(staged, mode):
    assert len(ct.refusal_lines(mode)) == len(ct.REFUSALS[mode][1]) + len(ct.REFUSALS[mode][2]) + 1
    assert ct.run_refusals(ct.CLI, staged, mode) == ct.golden("refusals_" + mode, "host")


def test_the_lines_reach_what_they_are_for():
    """two classes of epochs, two ages and a mask in the `mut --pairs` list; every fallback on its cursors; every refusal an error"""
    said = ct.golden("mut_pairs", "host")
    assert "Pair 3: 2e-05 " in said and "Pair 4 / 4: " in said
    assert "through the record cursors" in ct.golden("count_topo_cursors", "host")
    assert "through the record cursors" in ct.golden("compare_tmp_cursors", "host")
    assert "a sample has no walk index" in ct.golden("mut_interval_cursors", "host")
    for mode in ct.REFUSALS:
        text = ct.golden("refusals_" + mode, "host")
        assert text.count("exit 1\n") == len(ct.refusal_lines(mode)) and "exit 0" not in text
        assert text.count("cannot be combined with") == len(ct.refusal_lines(mode)) - 1
