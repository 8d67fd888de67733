"""GPU: `bce -t file archive.bce` -- the archive is decoded on the GPU and compared there with the file; nothing is written."""
import os
import subprocess

import pytest

import oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
DIFFERS = 1          # the usage text's "exit status 0 = equal, 1 = differs"


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _test(d, file, arc):
    """`bce -t`, with the directory's listing taken before and after: nothing may be written."""
    before = _listing(d)
    r = _bce("-t", file, arc)
    assert _listing(d) == before
    return r


def test_compress_then_test(tmp_path):
    data = oracle.synth_text(12, 300000)
    src, arc = tmp_path / "in.txt", tmp_path / "a.bce"
    src.write_bytes(data)
    r = _bce("-c", arc, src)
    assert r.returncode == 0, r.stdout + r.stderr
    assert arc.read_bytes() == oracle.compress(data)
    r = _test(tmp_path, src, arc)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("BCE v0.4 Release\n")
    assert "Archive OK: %d B -> 300000 B in " % arc.stat().st_size in r.stdout

    # one byte of the file changed
    for at in (0, 123457, 299999):
        bad = bytearray(data)
        bad[at] ^= 1
        src.write_bytes(bad)
        r = _test(tmp_path, src, arc)
        assert r.returncode == DIFFERS, r.stdout + r.stderr
        assert "Archive differs from file at byte %d\n" % at in r.stdout
        assert "Archive OK" not in r.stdout

    # another size: reported as such
    src.write_bytes(data[:-10])
    r = _test(tmp_path, src, arc)
    assert r.returncode == DIFFERS and "Archive differs from file in size: the archive holds 300000 B, the file 299990 B" in r.stdout, r.stdout
    src.write_bytes(data + b"more")
    r = _test(tmp_path, src, arc)
    assert r.returncode == DIFFERS and "Archive differs from file in size: the archive holds 300000 B, the file 300004 B" in r.stdout, r.stdout
    # ... unless the bytes that are there already differ
    bad = bytearray(data + b"more")
    bad[77] ^= 0x80
    src.write_bytes(bad)
    r = _test(tmp_path, src, arc)
    assert r.returncode == DIFFERS and "Archive differs from file at byte 77\n" in r.stdout, r.stdout


def test_container_reports_the_offset_within_the_whole_file(tmp_path):
    data = oracle.synth_text(13, 400001) + oracle.synth_rand(13, 50000)
    n = len(data)
    src, arc = tmp_path / "in.bin", tmp_path / "a.bcem"
    src.write_bytes(data)
    r = _bce("-c4", arc, src)
    assert r.returncode == 0, r.stdout + r.stderr
    assert arc.read_bytes()[:4] == b"BCEM"
    r = _test(tmp_path, src, arc)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Archive OK: %d B -> %d B in " % (arc.stat().st_size, n) in r.stdout
    # the third of four blocks: [2 * base + min(2, rem), ...) with base = n // 4, rem = n % 4
    base, rem = n // 4, n % 4
    lo, hi = 2 * base + min(2, rem), 3 * base + min(3, rem)
    for at in (lo, lo + (hi - lo) // 2, hi - 1):
        bad = bytearray(data)
        bad[at] ^= 0x10
        src.write_bytes(bad)
        r = _test(tmp_path, src, arc)
        assert r.returncode == DIFFERS, r.stdout + r.stderr
        assert "Archive differs from file at byte %d\n" % at in r.stdout
    src.write_bytes(data[:lo + 5])
    r = _test(tmp_path, src, arc)
    assert r.returncode == DIFFERS and "Archive differs from file in size: the archive holds %d B, the file %d B" % (n, lo + 5) in r.stdout, r.stdout


def test_truncated_and_missing_archives(tmp_path):
    data = oracle.synth_text(14, 200000)
    src, arc = tmp_path / "in.txt", tmp_path / "a.bce"
    src.write_bytes(data)
    full = oracle.compress(data)
    arc.write_bytes(full[:len(full) // 2])
    r = _test(tmp_path, src, arc)
    assert r.returncode not in (0, DIFFERS), r.stdout + r.stderr
    assert "Decompression failed: " in r.stdout and "Archive OK" not in r.stdout
    arc.write_bytes(full[:3])
    r = _test(tmp_path, src, arc)
    assert r.returncode not in (0, DIFFERS) and "Archive OK" not in r.stdout
    r = _test(tmp_path, src, tmp_path / "nope.bce")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    arc.write_bytes(full)
    r = _test(tmp_path, tmp_path / "nope.txt", arc)
    assert r.returncode == 255 and "Error loading file" in r.stdout
    r = _test(tmp_path, src, arc)
    assert r.returncode == 0 and "Archive OK: %d B -> 200000 B in " % len(full) in r.stdout
