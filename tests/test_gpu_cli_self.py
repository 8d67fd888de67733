"""GPU: `bce -gz MINLEN file` and `bce -gzd MINLEN archive` -- the one line of the self-parse on a file, a plain archive and a -C2
container, against the chain of tests/lpf_ref.py at the command's bounds (MINLEN .. max(256, MINLEN))."""
import os
import subprocess

import pytest

import bce_amd
from conftest import ROOT

import lpf_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("self_cli")
    t = bce_amd.synth_text(33, 9000).tobytes()
    data = t[:6000] + t[1000:4000] + t[6000:] + b"a" * 700                # a pasted slice and a run
    (d / "text").write_bytes(data)
    (d / "one").write_bytes(b"x")
    for flag, name in (("-c", "plain.bce"), ("-C2", "checked.bcem")):
        r = subprocess.run([EXE, flag, str(d / name), str(d / "text")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout
    before = sorted(os.listdir(str(d)))

    def run(*args):
        r = subprocess.run([EXE] + [str(d / a) if isinstance(a, str) and not a.startswith("-") else str(a) for a in args], capture_output=True, text=True, cwd=str(d))
        assert sorted(os.listdir(str(d))) == before                       # writes nothing
        lines = r.stdout.split("\n")
        return lines[lines.index("") + 1:], r.returncode

    return run, data


@pytest.mark.parametrize("min_len", (1, 16, 300))
def test_the_line_is_the_reference_chain_on_a_file_an_archive_and_a_container(box, min_len):
    run, data = box
    want = ref.summary_line(data, min_len, max(256, min_len))
    for args in (("-gz", min_len, "text"), ("-gzd", min_len, "plain.bce"), ("-gzd", min_len, "checked.bcem")):
        lines, code = run(*args)
        assert code == 0 and lines == [want, ""], (args, lines)
    assert " phrases at bounds %d .. %d; " % (min_len, max(256, min_len)) in want and want.endswith(" of %d bytes repeat earlier text" % len(data))


def test_a_text_of_one_byte(box):
    run, _data = box
    lines, code = run("-gz", 4, "one")
    assert code == 0 and lines == ["0 copies of 0 bytes, 1 literal bytes in 1 runs: 1 phrases at bounds 4 .. 256; 0 of 1 bytes repeat earlier text", ""]
