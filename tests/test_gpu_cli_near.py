"""GPU: `bce -gn K PATTERN file`, `-gnd K PATTERN archive`, `-gnl` and `-gnld` -- what a sliding window over the bytes finds within K
mismatches: one line per distance and the sum, or "POS d" per hit in ascending position; from the index K1 and K2 build on the GPU;
nothing is written.  Compared line for line with output built from tests/near_ref.py."""
import os
import subprocess

import pytest

from conftest import ROOT

import near_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
DATA = b"abracadabra" * 100
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def test_the_four_commands_on_a_file_an_archive_and_a_checked_container(tmp_path):
    src, arc, blob = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem"
    src.write_bytes(DATA)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "abra", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    for pattern, k, archives in (("abra", 2, True), ("aabr", 0, False), ("abrx", 1, True), ("x", 1, False)):
        counts = ref.counts(DATA, pattern.encode(), k, cyclic=False).tolist()
        pos, dist = ref.hits(DATA, pattern.encode(), k, cyclic=False)
        tail = ["%d occurrences" % sum(counts), ""]
        want_n = "\n".join(banner + ["distance %d: %d" % (d, c) for d, c in enumerate(counts)] + tail)
        want_l = "\n".join(banner + ["%d %d" % (p, d) for p, d in zip(pos.tolist(), dist.tolist())] + tail)
        for files in ((src, ""), (arc, "d"), (blob, "d"))[:3 if archives else 1]:
            r = _bce("-gn" + files[1], k, pattern, files[0])
            assert r.returncode == 0 and r.stdout == want_n, (k, pattern, files, r.stdout + r.stderr)
            r = _bce("-gnl" + files[1], k, pattern, files[0])
            assert r.returncode == 0 and r.stdout == want_l, (k, pattern, files, r.stdout + r.stderr)
    # the 100th "aabr" runs across the end: not a hit of the window; with K = 0 the answers are -g's and -gl's
    assert ref.counts(DATA, b"aabr", 0, cyclic=True)[0] == 100 and ref.counts(DATA, b"aabr", 0, cyclic=False)[0] == 99
    assert _bce("-gnl", 0, "aabr", src).stdout.split("\n")[-2] == _bce("-g", "aabr", src).stdout.split("\n")[-2] == "99 occurrences"
    r = _bce("-gn", 2, "abra" * 300, src)                               # longer than the file: nowhere
    assert r.returncode == 0 and r.stdout == "\n".join(banner + ["distance 0: 0", "distance 1: 0", "distance 2: 0", "0 occurrences", ""])
    r = _bce("-gnl", 2, "abra" * 300, src)
    assert r.returncode == 0 and r.stdout == "\n".join(banner + ["0 occurrences", ""])
    assert _listing(tmp_path) == before


def test_missing_and_damaged_inputs_give_the_existing_error_exits(tmp_path):
    for cmd in ("-gn", "-gnl"):
        r = _bce(cmd, 1, "abra", tmp_path / "missing")
        assert r.returncode == 255 and "Error loading file" in r.stdout and "occurrences" not in r.stdout
        r = _bce(cmd + "d", 1, "abra", tmp_path / "missing")
        assert r.returncode == 255 and "Archive not found." in r.stdout
    src, blob = tmp_path / "in.txt", tmp_path / "a.bcem"
    src.write_bytes(DATA)
    assert _bce("-C2", blob, src).returncode == 0
    bad = bytearray(blob.read_bytes())
    bad[12 + 16] ^= 1                                                    # one flipped text CRC: the mismatch -d reports, no answer
    blob.write_bytes(bad)
    for cmd in ("-gnd", "-gnld"):
        r = _bce(cmd, 1, "abra", blob)
        assert r.returncode == 252 and "Checksum mismatch in block 0" in r.stdout and "occurrences" not in r.stdout
    r = _bce("-gn", 1, "e" * 5000, src)                                  # longer than the file: answered before the bound on m is met
    assert r.returncode == 0 and "0 occurrences" in r.stdout
