"""GPU: `bce -gm MINLEN file query_file` and `bce -gmd MINLEN archive query_file` -- one line that says how many bytes of the query
file lie in strings of MINLEN bytes or more that occur in the file, or in what the archive holds; searched and reduced on the GPU;
nothing is written."""
import os
import re
import subprocess

import pytest

import bce_amd
from conftest import ROOT

import match_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def test_coverage_of_a_query_file_in_a_file_an_archive_and_both_container_kinds(tmp_path):
    data = bce_amd.synth_text(23, 9000).tobytes()
    query = bytearray(data[3000:5000] + b"abracadabra" * 20 + data[-40:] + data[:40])
    for at in range(29, 2000, 131):
        query[at] ^= 0x80
    query = bytes(query)
    src, qf, arc, blob, plain = tmp_path / "in.txt", tmp_path / "query.bin", tmp_path / "a.bce", tmp_path / "a.bcem", tmp_path / "b.bcem"
    src.write_bytes(data)
    qf.write_bytes(query)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0 and _bce("-c3", plain, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "the", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    seen = set()
    for m in (1, 16, 100):
        want = ref.coverage(data, query, m)
        seen.add(want)
        for args in (("-gm", m, src, qf), ("-gmd", m, arc, qf), ("-gmd", m, blob, qf), ("-gmd", m, plain, qf)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            line = "%d of %d bytes (%.1f %%) of %s lie in strings of %d bytes or more that occur in %s" % (
                want, len(query), 100.0 * want / len(query), qf, m, args[2])
            assert r.stdout == "\n".join(banner + [line, ""]), (args, r.stdout)
    assert len(seen) == 3 and 0 < min(seen) and max(seen) < len(query)
    # the other way round, two small files: the indexed one shorter than the matches asked for
    r = _bce("-gm", 4096, qf, src)
    assert r.returncode == 0 and re.search(r"^0 of 9000 bytes \(0\.0 %\) of ", r.stdout, flags=re.M)
    assert _listing(tmp_path) == before


def test_missing_and_empty_inputs_give_the_count_commands_exits(tmp_path):
    src, qf, empty = tmp_path / "in.txt", tmp_path / "query.bin", tmp_path / "empty"
    src.write_bytes(b"abracadabra" * 100)
    qf.write_bytes(b"cadabra abra")
    empty.write_bytes(b"")
    r = _bce("-gm", 4, tmp_path / "missing", qf)
    assert r.returncode == 255 and "Error loading file" in r.stdout and " lie in " not in r.stdout
    r = _bce("-gmd", 4, tmp_path / "missing", qf)
    assert r.returncode == 255 and "Archive not found." in r.stdout
    assert _bce("-gm", 4, empty, qf).returncode == 255 and _bce("-gmd", 4, empty, qf).returncode == 254
    for query in (tmp_path / "missing", empty):
        r = _bce("-gm", 4, src, query)
        assert r.returncode == 255 and "Error loading file" in r.stdout and " lie in " not in r.stdout
    r = _bce("-gm", 4, src, qf)
    assert r.returncode == 0 and "11 of 12 bytes (91.7 %)" in r.stdout     # "cadabra" and "abra" occur, the blank does not
