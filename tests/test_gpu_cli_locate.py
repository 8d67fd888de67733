"""GPU: `bce -gl PATTERN file` and `bce -gld PATTERN archive` -- the byte offsets an overlapping scan of the bytes finds, one per
line, ascending, then -g's count line; from the index and the suffix array K1 and K2 build on the GPU; nothing is written."""
import os
import subprocess

import pytest

from conftest import ROOT

import locate_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
DATA = b"abracadabra" * 100
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def test_locate_in_a_file_an_archive_and_both_container_kinds(tmp_path):
    src, arc, blob, plain = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem", tmp_path / "b.bcem"
    src.write_bytes(DATA)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0 and _bce("-c3", plain, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "abra", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    for pattern in ("abra", "aabr", "x", "a"):
        want = ref.linear_hits(DATA, pattern.encode())
        for args in (("-gl", pattern, src), ("-gld", pattern, arc), ("-gld", pattern, blob), ("-gld", pattern, plain)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            assert r.stdout == "\n".join(banner + [str(v) for v in want] + ["%d occurrences" % len(want), ""]), (args, r.stdout)
        # -g's own line is what it was
        assert _bce("-g", pattern, src).stdout == "\n".join(banner + ["%d occurrences" % len(want), ""])
    assert len(ref.linear_hits(DATA, b"abra")) == 200 and len(ref.linear_hits(DATA, b"aabr")) == 99   # (the 100th "aabr" runs across the end)
    r = _bce("-gl", "abra" * 300, src)                                   # longer than the file: no offset lines
    assert r.returncode == 0 and r.stdout == "\n".join(banner + ["0 occurrences", ""])
    assert _listing(tmp_path) == before


def test_missing_and_damaged_inputs_give_the_existing_error_exits(tmp_path):
    r = _bce("-gl", "abra", tmp_path / "missing")
    assert r.returncode == 255 and "Error loading file" in r.stdout and "occurrences" not in r.stdout
    r = _bce("-gld", "abra", tmp_path / "missing")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    assert _bce("-gl", "abra", empty).returncode == 255 and _bce("-gld", "abra", empty).returncode == 254
    # a container with one flipped text CRC: the mismatch -d reports, no offsets and no count
    src, blob = tmp_path / "in.txt", tmp_path / "a.bcem"
    src.write_bytes(DATA)
    assert _bce("-C2", blob, src).returncode == 0
    bad = bytearray(blob.read_bytes())
    bad[12 + 16] ^= 1
    blob.write_bytes(bad)
    r = _bce("-gld", "abra", blob)
    assert r.returncode == 252 and "Checksum mismatch in block 0" in r.stdout and "occurrences" not in r.stdout
    assert r.stdout == _bce("-gd", "abra", blob).stdout
