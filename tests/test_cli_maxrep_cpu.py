"""CPU: what `bce -gp ORDER MINLEN N file` / `-gpd ORDER MINLEN N archive` judge before they need a device -- the arguments that end
in the usage text, the indexed file or archive, then the device -- and their two paragraphs of the usage text."""
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("maxrep_cli")
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


def test_bad_order_minlen_and_n_end_in_the_usage_text(box):
    for args in (("-gp",), ("-gp", "len"), ("-gp", "len", 4), ("-gp", "len", 4, 5), ("-gp", "len", 4, 5, "text", "x"), ("-gp", "size", 4, 5, "text"),
                 ("-gp", "LEN", 4, 5, "text"), ("-gp", "", 4, 5, "text"), ("-gp", 0, 4, 5, "text"), ("-gp", "len", 0, 5, "text"),
                 ("-gp", "len", 4097, 5, "text"), ("-gp", "len", 4, 0, "text"), ("-gp", "len", 4, 65537, "text"), ("-gp", "len", "4x", 5, "text"),
                 ("-gp", "len", 4, "5x", "text"), ("-gp", "len", "", 5, "text"), ("-gp", "len", 4, "", "text"), ("-gp", "len", "+4", 5, "text"),
                 ("-gp", "len", -1, 5, "text"), ("-gp", "len", 4, "5.0", "text"), ("-gp", "len", 99999999999, 5, "text"), ("-gpx", "len", 4, 5, "text"),
                 ("-gpd", "len", 4, 5), ("-gpd", "gains", 4, 5, "text"), ("-gpd", "count", 0, 5, "text"), ("-gpd", "count", 4, 65537, "text")):
        assert box(*args) == ("Usage:", 0), args


def test_the_indexed_file_or_archive_is_judged_before_the_device(box):
    for order in ("len", "count", "gain"):
        for indexed in ("missing", "empty"):
            assert box("-gp", order, 4, 5, indexed) == ("Error loading file", 255)
        assert box("-gpd", order, 4, 5, "missing") == ("Archive not found.", 255)
        assert box("-gpd", order, 4, 5, "empty") == ("Could not read Archive.", 254)
    for m, N in ((1, 1), (4096, 65536)):                                  # the bounds themselves are sound
        assert box("-gp", "gain", m, N, "missing") == ("Error loading file", 255)


def test_usage_has_the_two_paragraphs_and_keeps_the_top_kgrams_ones_last():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gp ORDER MINLEN N file")
    assert lines[at - 1] == "" and lines[at + 1].startswith("   ") and lines[at + 2] == ""
    assert lines[at + 3] == "  bce -gpd ORDER MINLEN N archive.bce" and lines[at + 4].startswith("   ") and lines[at + 5] == ""
    for word in ("1..65536", "1..4096", "len", "count", "gain", "4096+", "\\xHH", "BWT"):
        assert word in lines[at + 1], word
    assert lines.index("  bce -gfd K N archive.bce") == len(lines) - 3 and at < lines.index("  bce -gf K N file")
