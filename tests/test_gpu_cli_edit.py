"""GPU: `bce -gw K PATTERN file`, `-gwd K PATTERN archive`, `-gwl` and `-gwld` -- the positions of the bytes where something starts
within K edits of PATTERN, over the alignments that end inside the file: one line per distance and the sum, or "POS LEN d" per hit in
ascending position; from the index and the suffix array K1 and K2 build on the GPU; nothing is written.  Compared line for line with
output built from tests/edit_ref.py."""
import os
import subprocess

import pytest

from conftest import ROOT

import edit_ref as ref

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
    for pattern, k, archives in (("abracadabra", 2, True), ("abrcadabra", 1, True), ("abraacadabra", 1, False), ("aabr", 0, False), ("x", 1, False)):
        pos, lens, dist = ref.hits(DATA, pattern.encode(), k, cyclic=False)
        counts = ref.counts_of(dist, k).tolist()
        tail = ["%d occurrences" % sum(counts), ""]
        want_n = "\n".join(banner + ["distance %d: %d" % (d, c) for d, c in enumerate(counts)] + tail)
        want_l = "\n".join(banner + ["%d %d %d" % v for v in zip(pos.tolist(), lens.tolist(), dist.tolist())] + tail)
        for files in ((src, ""), (arc, "d"), (blob, "d"))[:3 if archives else 1]:
            r = _bce("-gw" + files[1], k, pattern, files[0])
            assert r.returncode == 0 and r.stdout == want_n, (k, pattern, files, r.stdout + r.stderr)
            r = _bce("-gwl" + files[1], k, pattern, files[0])
            assert r.returncode == 0 and r.stdout == want_l, (k, pattern, files, r.stdout + r.stderr)
    # a byte dropped from the pattern: found at distance 1 with the text's length, one byte more than the pattern's
    assert _bce("-gwl", 1, "abrcadabra", src).stdout.split("\n")[BANNER_LINES] == "0 11 1"
    # the 100th "aabr" runs across the end; with K = 0 the answers are -g's and -gl's
    assert _bce("-gwl", 0, "aabr", src).stdout.split("\n")[-2] == _bce("-g", "aabr", src).stdout.split("\n")[-2] == "99 occurrences"
    # the last hit ends inside the file: "bracadabra" at n - 10; the circular text's (n - 1, 12, 1) is not a hit of the file
    assert ref.hits(DATA, b"abracadabra", 2, cyclic=True)[0][-1] == len(DATA) - 1
    assert _bce("-gwl", 2, "abracadabra", src).stdout.split("\n")[-3] == "%d 10 2" % (len(DATA) - 10)
    assert _listing(tmp_path) == before


def test_missing_and_damaged_inputs_give_the_existing_error_exits(tmp_path):
    for cmd in ("-gw", "-gwl"):
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
    for cmd in ("-gwd", "-gwld"):
        r = _bce(cmd, 1, "abra", blob)
        assert r.returncode == 252 and "Checksum mismatch in block 0" in r.stdout and "occurrences" not in r.stdout
    r = _bce("-gw", 1, "e" * 5000, src)                                  # over the bound on m: the call's refusal, the index queries' exit
    assert r.returncode == 252 and "Count failed" in r.stdout and "4096" in r.stdout
