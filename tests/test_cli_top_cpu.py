"""CPU: what `bce -gf K N file` / `-gfd K N archive` judge before they need a device -- the arguments that end in the usage text, the
indexed file or archive, then the device -- and their two paragraphs of the usage text."""
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("top_cli")
    (d / "text").write_bytes(b"abracadabra" * 100)
    (d / "empty").write_bytes(b"")
    work = d / "work"
    work.mkdir()

    def run(*args):
        """(first line behind the banner and its blank line, exit status) of `bce args`, run in an empty directory"""
        argv = [str(d / a) if a in ("text", "empty", "missing") else str(a) for a in args]
        r = subprocess.run([EXE] + argv, capture_output=True, text=True, cwd=str(work))
        assert os.listdir(str(work)) == [], (args, os.listdir(str(work)))
        lines = r.stdout.split("\n")
        return lines[lines.index("") + 1], r.returncode

    return run


def test_bad_k_and_n_end_in_the_usage_text(box):
    for args in (("-gf",), ("-gf", 4), ("-gf", 4, 5), ("-gf", 4, 5, "text", "x"), ("-gf", 0, 5, "text"), ("-gf", 257, 5, "text"), ("-gf", 4, 0, "text"),
                 ("-gf", 4, 65537, "text"), ("-gf", "4x", 5, "text"), ("-gf", 4, "5x", "text"), ("-gf", "", 5, "text"), ("-gf", 4, "", "text"),
                 ("-gf", "+4", 5, "text"), ("-gf", " 4", 5, "text"), ("-gf", -1, 5, "text"), ("-gf", 4, "5.0", "text"), ("-gf", 99999999999, 5, "text"),
                 ("-gfx", 4, 5, "text"), ("-gfd", 4, 5), ("-gfd", 0, 5, "text"), ("-gfd", 4, 65537, "text")):
        assert box(*args) == ("Usage:", 0), args


def test_the_indexed_file_or_archive_is_judged_before_the_device(box):
    for indexed in ("missing", "empty"):
        assert box("-gf", 4, 5, indexed) == ("Error loading file", 255)
    assert box("-gfd", 4, 5, "missing") == ("Archive not found.", 255)
    assert box("-gfd", 4, 5, "empty") == ("Could not read Archive.", 254)
    for K, N in ((1, 1), (256, 65536)):                                   # the bounds themselves are sound
        line, code = box("-gf", K, N, "missing")
        assert (line, code) == ("Error loading file", 255)


def test_usage_has_the_two_paragraphs_at_its_end():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gad archive.bce in.bcd out_file")
    assert lines[at + 2] == "" and lines[at + 3] == "  bce -gf K N file" and lines[at + 4].startswith("   ")
    assert lines[at + 5] == "" and lines[at + 6] == "  bce -gfd K N archive.bce" and lines[at + 7].startswith("   ")
    assert lines[at + 8:] == [""] and "1..65536" in lines[at + 4] and "1..256" in lines[at + 4] and "\\xHH" in lines[at + 4]
