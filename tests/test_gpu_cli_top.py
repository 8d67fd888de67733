"""GPU: `bce -gf K N file` and `bce -gfd K N archive` -- a head line, then the N most frequent K-grams of the circular text as
`count pos ESCAPED`, then `D distinct, n bytes`: count and bytes line for line what Python formats from tests/top_ref.py, the
position checked (its cyclic cut is the K-gram); nothing is written."""
import os
import subprocess

import pytest

import bce_amd
from conftest import ROOT

import top_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def _check(data, K, N, stdout, banner=None):
    lines = stdout.split("\n")
    if banner is not None:
        assert lines[:BANNER_LINES] == banner
    want, distinct, _ = ref.top_kgrams(data, K, N)
    body = lines[BANNER_LINES:]
    assert body[0] == "most frequent %d-grams of the circular text: count position bytes" % K
    assert len(body) == len(want) + 3 and body[-2:] == ["%d distinct, %d bytes" % (distinct, len(data)), ""], stdout[-300:]
    ext = data * (K // len(data) + 2)
    for line, (count, _, gram) in zip(body[1:], want):
        w = line.split(" ")
        assert len(w) == 3 and w[0] == str(count) and w[2] == ref.escape(gram), (line, count, gram)
        assert 0 <= int(w[1]) < len(data) and ext[int(w[1]):int(w[1]) + K] == gram, line


def test_the_list_of_a_file_an_archive_and_both_container_kinds(tmp_path):
    data = bce_amd.synth_text(23, 9000).tobytes()
    src, arc, blob, plain = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem", tmp_path / "b.bcem"
    src.write_bytes(data)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C2", blob, src).returncode == 0 and _bce("-c2", plain, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "the", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    for K, N in ((4, 10), (1, 65536), (256, 3)):
        for args in (("-gf", K, N, src), ("-gfd", K, N, arc), ("-gfd", K, N, blob), ("-gfd", K, N, plain)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            _check(data, K, N, r.stdout, banner)
    assert _listing(tmp_path) == before


def test_bytes_that_are_escaped_ties_and_texts_shorter_than_k(tmp_path):
    cases = {"periodic": b"ab" * 150, "one": b"z", "all": bytes(range(256)) * 2, "blank": b"a b\\c\n" * 20 + b"\x00\xff\x7f"}
    for name, data in cases.items():
        f = tmp_path / name
        f.write_bytes(data)
        for K, N in ((1, 300), (3, 5), (7, 65536)):
            r = _bce("-gf", K, N, f)
            assert r.returncode == 0, r.stdout + r.stderr
            _check(data, K, N, r.stdout)
    r = _bce("-gf", 3, 9, tmp_path / "periodic")
    assert r.stdout.split("\n")[BANNER_LINES + 1:BANNER_LINES + 4][0].split(" ")[::2] == ["150", "aba"]      # the tie: `ab...` first
    assert r.stdout.split("\n")[BANNER_LINES + 2].split(" ")[::2] == ["150", "bab"] and r.stdout.endswith("2 distinct, 300 bytes\n")
    r = _bce("-gf", 2, 1, tmp_path / "blank")
    assert r.stdout.split("\n")[BANNER_LINES + 1].split(" ")[::2] == ["20", "\\x20b"]


def test_missing_and_empty_inputs_give_the_count_commands_exits(tmp_path):
    src, empty = tmp_path / "in.txt", tmp_path / "empty"
    src.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    r = _bce("-gf", 4, 5, tmp_path / "missing")
    assert r.returncode == 255 and "Error loading file" in r.stdout and "most frequent" not in r.stdout
    r = _bce("-gfd", 4, 5, tmp_path / "missing")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    assert _bce("-gf", 4, 5, empty).returncode == 255 and _bce("-gfd", 4, 5, empty).returncode == 254
    r = _bce("-gfd", 4, 5, src)                                           # not an archive: -gd's answer
    assert r.returncode == _bce("-gd", "abra", src).returncode != 0 and "most frequent" not in r.stdout
