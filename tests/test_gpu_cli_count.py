"""GPU: `bce -g PATTERN file` and `bce -gd PATTERN archive` -- the count an overlapping scan of the bytes gives, from the index
K1 and K2 build on the GPU; nothing is written."""
import os
import subprocess

import pytest

from conftest import ROOT

import count_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
DATA = b"abracadabra" * 100


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def test_count_in_a_file_an_archive_and_a_container(tmp_path):
    src, arc, blob = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem"
    src.write_bytes(DATA)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0
    before = _listing(tmp_path)
    for pattern in ("abra", "aabr", "x"):
        want = ref.linear_count(DATA, pattern.encode())
        for args in (("-g", pattern, src), ("-gd", pattern, arc), ("-gd", pattern, blob)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            assert r.stdout.startswith("BCE v0.4 Release\n") and r.stdout.endswith("\n%d occurrences\n" % want), (args, r.stdout)
    assert ref.linear_count(DATA, b"abra") == 200 and ref.linear_count(DATA, b"aabr") == 99       # (the 100th "aabr" runs across the end)
    r = _bce("-g", "abra" * 300, src)                                    # longer than the file
    assert r.returncode == 0 and r.stdout.endswith("\n0 occurrences\n")
    assert _listing(tmp_path) == before


def test_missing_and_damaged_inputs_give_the_existing_error_exits(tmp_path):
    r = _bce("-g", "abra", tmp_path / "missing")
    assert r.returncode == 255 and "Error loading file" in r.stdout and "occurrences" not in r.stdout
    r = _bce("-gd", "abra", tmp_path / "missing")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    assert _bce("-g", "abra", empty).returncode == 255 and _bce("-gd", "abra", empty).returncode == 254
    # a container with one flipped text CRC: the mismatch -d reports, no count
    src, blob = tmp_path / "in.txt", tmp_path / "a.bcem"
    src.write_bytes(DATA)
    assert _bce("-C2", blob, src).returncode == 0
    bad = bytearray(blob.read_bytes())
    bad[12 + 16] ^= 1
    blob.write_bytes(bad)
    r = _bce("-gd", "abra", blob)
    assert r.returncode == 252 and "Checksum mismatch in block 0" in r.stdout and "occurrences" not in r.stdout
