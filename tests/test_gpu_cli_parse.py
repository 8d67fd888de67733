"""GPU: `bce -gr MINLEN file query_file out.bcd` / `-grd` write a second file as a delta against a file or against what an archive
holds, `bce -ga file in.bcd out_file` / `-gad` rebuild it: the round trip byte for byte, the printed figures against
tests/parse_ref.py, the delta file against the Python reader, and the CRC-32 refusals on either side."""
import os

import pytest

import bce_amd
from bce_amd import container
from conftest import ROOT

import parse_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
K_EXIT_DIFFERS = 1


def _bce(*args):
    import subprocess
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _inputs(tmp_path):
    data = bce_amd.synth_text(23, 9000).tobytes()
    new = bytearray(data[3000:5000] + b"abracadabra" * 20 + data[-40:] + data[:40] + data[6000:8500])
    for at in range(29, len(new), 131):
        new[at] ^= 0x80
    src, qf = tmp_path / "in.txt", tmp_path / "new.bin"
    src.write_bytes(data)
    qf.write_bytes(bytes(new))
    return data, bytes(new), src, qf


def test_delta_then_apply_restores_the_file_against_a_file_an_archive_and_a_container(tmp_path):
    data, new, src, qf = _inputs(tmp_path)
    arc, blob = tmp_path / "a.bce", tmp_path / "a.bcem"
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C2", blob, src).returncode == 0
    for m in (4, 16, 300):
        L = max(256, m)
        ph, lits, info = ref.parse(data, new, m, L)
        size = 56 + 8 * info["nops"] + info["nlits"]
        line = "%d copies of %d bytes, %d literal bytes in %d runs: %d bytes of delta" % (
            info["ncopies"], info["copied"], info["nlits"], info["nops"] - info["ncopies"], size)
        for k, (make, apply, base) in enumerate((("-gr", "-ga", src), ("-grd", "-gad", arc), ("-grd", "-gad", blob))):
            bcd, out = tmp_path / ("d%d_%d.bcd" % (m, k)), tmp_path / ("out%d_%d" % (m, k))
            r = _bce(make, m, base, qf, bcd)
            assert r.returncode == 0 and line in r.stdout.split("\n"), (make, m, r.stdout + r.stderr)
            d = container.unpack_delta(bcd.read_bytes())
            assert bcd.stat().st_size == size and (d["n"], d["q"], d["min_len"], d["max_len"]) == (len(data), len(new), m, L)
            assert d["base_crc"] == bce_amd.crc32(data) and d["crc"] == bce_amd.crc32(new)
            ref.check(data, new, (ph, lits, info), d["ops"], d["lits"], info)
            r = _bce(apply, base, bcd, out)
            assert r.returncode == 0, (apply, r.stdout + r.stderr)
            assert out.read_bytes() == new
    assert bce_amd.apply_delta(data, (tmp_path / "d16_0.bcd").read_bytes()) == new                # the library reads the CLI's file
    (tmp_path / "py.bcd").write_bytes(bce_amd.delta(data, new))                                   # and the CLI the library's
    assert _bce("-ga", src, tmp_path / "py.bcd", tmp_path / "out_py").returncode == 0 and (tmp_path / "out_py").read_bytes() == new


def test_a_changed_base_or_a_lying_delta_gives_the_differs_exit_and_no_file(tmp_path):
    data, new, src, qf = _inputs(tmp_path)
    bcd, out = tmp_path / "d.bcd", tmp_path / "out"
    assert _bce("-gr", 16, src, qf, bcd).returncode == 0
    wrong = bytearray(data)
    wrong[4321] ^= 1
    other, shorter = tmp_path / "other.txt", tmp_path / "shorter.txt"
    other.write_bytes(bytes(wrong))
    shorter.write_bytes(data[:-1])
    for base in (other, shorter):
        r = _bce("-ga", base, bcd, out)
        assert r.returncode == K_EXIT_DIFFERS and not out.exists(), r.stdout
    lied = bytearray(bcd.read_bytes())
    lied[28] ^= 1                                                         # the result's CRC-32
    (tmp_path / "lied.bcd").write_bytes(bytes(lied))
    r = _bce("-ga", src, tmp_path / "lied.bcd", out)
    assert r.returncode == K_EXIT_DIFFERS and "Checksum mismatch" in r.stdout and not out.exists()
    lied = bytearray(bcd.read_bytes())
    lied[56] ^= 0xFF                                                      # the first op's length: the list no longer adds up
    (tmp_path / "bad.bcd").write_bytes(bytes(lied))
    r = _bce("-ga", src, tmp_path / "bad.bcd", out)
    assert r.returncode != 0 and not out.exists()
    for bad in (bcd.read_bytes()[:-1], bcd.read_bytes()[:40], b"", b"BCEM" + bcd.read_bytes()[4:]):
        (tmp_path / "cut.bcd").write_bytes(bad)
        r = _bce("-ga", src, tmp_path / "cut.bcd", out)
        assert r.returncode == 254 and "Could not read Archive." in r.stdout and not out.exists()
    r = _bce("-ga", src, tmp_path / "missing.bcd", out)
    assert r.returncode == 255 and "Archive not found." in r.stdout
    assert _bce("-ga", src, bcd, out).returncode == 0 and out.read_bytes() == new
