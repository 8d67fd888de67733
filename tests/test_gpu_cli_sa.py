"""GPU: `bce -gs`, `-gsd` and `-gsc` -- the suffix array of a file or of what a plain archive holds as native 32-bit words, and the
check of such a file against its text."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import sa_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


def bce(*args):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)
    lines = r.stdout.split("\n")
    return r.returncode, lines[lines.index("") + 1:], r


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_cli_gpu")
    data = oracle.synth_text(12, 70001)
    (d / "text").write_bytes(data)
    code, lines, r = bce("-gs", d / "text", d / "text.sa")
    assert code == 0 and lines[0] == "70001 suffixes", r.stdout + r.stderr
    return d, data


def test_gs_writes_the_array_and_gsc_accepts_it(box):
    d, data = box
    sa = np.fromfile(str(d / "text.sa"), dtype=np.uint32)
    assert np.array_equal(sa, sa_ref.suffix_array(data).view(np.uint32))
    code, lines, r = bce("-gsc", d / "text", d / "text.sa")
    assert code == 0 and lines[0] == "70001 suffixes in order", r.stdout + r.stderr


def test_gsc_names_the_row_of_a_swap_and_the_other_reasons(box):
    d, data = box
    sa = np.fromfile(str(d / "text.sa"), dtype=np.uint32)
    for name, edit, word in (("swap.sa", "swap", "Out of order: row "), ("range.sa", "range", "Out of range: row "), ("twice.sa", "twice", "Not a permutation: no row holds position ")):
        m = sa.copy()
        if edit == "swap":
            m[[40000, 40001]] = m[[40001, 40000]]
        elif edit == "range":
            m[69999] = 70001
        else:
            m[5] = m[6]
        m.tofile(str(d / name))
        reason, at = sa_ref.check(data, m)
        code, lines, r = bce("-gsc", d / "text", d / name)
        assert code == 1 and lines[0].startswith(word + "%d" % at), (lines[0], reason, at)
        assert not lines[0][len(word) + len(str(at)):][:1].isdigit()


def test_gsd_on_a_plain_archive_is_gs_on_the_original(box):
    d, data = box
    code, _, r = bce("-c", d / "text.bce", d / "text")
    assert code == 0, r.stdout + r.stderr
    code, lines, r = bce("-gsd", d / "text.bce", d / "arch.sa")
    assert code == 0 and lines[0] == "70001 suffixes", r.stdout + r.stderr
    assert (d / "arch.sa").read_bytes() == (d / "text.sa").read_bytes()


def test_gsd_refuses_a_container(box):
    d, data = box
    code, _, r = bce("-c2", d / "text.bcem", d / "text")
    assert code == 0, r.stdout + r.stderr
    code, lines, r = bce("-gsd", d / "text.bcem", d / "none.sa")
    assert code == 254 and lines[0].startswith("A container holds separate texts") and not (d / "none.sa").exists()


def test_a_failed_write_is_an_error_and_leaves_no_file(box):
    d, data = box
    code, lines, r = bce("-gs", d / "text", d / "no_such_dir" / "out.sa")
    assert code == 251 and lines[0] == "Could not write file." and not (d / "no_such_dir").exists()
