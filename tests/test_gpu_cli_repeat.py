"""GPU: `bce -gk K file` and `bce -gkd K archive` -- for k = 0..K the distinct k-grams of the circular text, those that occur once,
the most frequent one's occurrences and H_k, then the longest repeat and the size: line for line what Python formats from the
references of tests/repeat_ref.py with the same double expression; nothing is written."""
import os
import subprocess

import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import repeat_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def _table(data, K):
    """The lines between the banner and the longest repeat."""
    n = len(data)
    recs = [ref.kgram_record(data, k, lambda c: api.cost_q24(1, c)) for k in range(K + 2)]
    lines = ["k-grams of the circular text: k distinct once most H_k"]
    for k in range(K + 1):
        distinct, once, s_k, most = recs[k]
        lines.append("%u %u %u %u %.6f" % (k, distinct, once, most, ref.entropy_q24(n, s_k, recs[k + 1][2])))
    return lines


def _check_repeat_line(data, line):
    """`longest repeat: L bytes at A and B`: L is the largest capped LCP, and the two rotations agree on exactly L bytes."""
    top = int(ref.capped_lcp(data, 4096).max())
    w = line.split()
    if top == 0:
        assert line == "longest repeat: none"
        return
    more = top == 4096
    assert w[:2] == ["longest", "repeat:"] and int(w[2]) == top
    assert w[3:] == (["or", "more", "bytes", "at", w[-3], "and", w[-1]] if more else ["bytes", "at", w[-3], "and", w[-1]]), line
    a, b = int(w[-3]), int(w[-1])
    assert a != b and max(a, b) < len(data) and ref.rot_lcp(data, a, b, 4096) == top


def test_kgram_table_of_a_file_an_archive_and_both_container_kinds(tmp_path):
    data = bce_amd.synth_text(23, 9000).tobytes()
    src, arc, blob, plain = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem", tmp_path / "b.bcem"
    src.write_bytes(data)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0 and _bce("-c2", plain, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "the", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    for K in (4, 0):
        table = _table(data, K)
        assert len(table) == K + 2
        for args in (("-gk", K, src), ("-gkd", K, arc), ("-gkd", K, blob), ("-gkd", K, plain)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            lines = r.stdout.split("\n")
            assert lines[:BANNER_LINES] == banner and lines[BANNER_LINES:BANNER_LINES + K + 2] == table, (args, r.stdout)
            assert lines[BANNER_LINES + K + 3:] == ["9000 bytes", ""], (args, r.stdout)
            _check_repeat_line(data, lines[BANNER_LINES + K + 2])
    assert float(_table(data, 4)[1].split()[-1]) > float(_table(data, 4)[5].split()[-1]) > 0       # H_0 > H_4 > 0 on text
    assert _listing(tmp_path) == before


def test_periodic_single_byte_and_repeat_free_texts(tmp_path):
    cases = {"periodic": b"ab" * 150, "one": b"z", "free": bytes(range(256)),
             "long": bce_amd.synth_rand(12, 5000).tobytes() * 2}           # the repeat passes the bound: "4096 or more"
    for name, data in cases.items():
        f = tmp_path / name
        f.write_bytes(data)
        r = _bce("-gk", 2, f)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        assert lines[BANNER_LINES:BANNER_LINES + 4] == _table(data, 2), (name, r.stdout)
        assert lines[BANNER_LINES + 5:] == ["%d bytes" % len(data), ""]
        _check_repeat_line(data, lines[BANNER_LINES + 4])
        if name in ("one", "free"):
            assert lines[BANNER_LINES + 4] == "longest repeat: none"
        if name in ("periodic", "long"):
            assert lines[BANNER_LINES + 4].startswith("longest repeat: 4096 or more bytes at ")


def test_missing_and_empty_inputs_give_the_count_commands_exits(tmp_path):
    src, empty = tmp_path / "in.txt", tmp_path / "empty"
    src.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    r = _bce("-gk", 4, tmp_path / "missing")
    assert r.returncode == 255 and "Error loading file" in r.stdout and "k-grams" not in r.stdout
    r = _bce("-gkd", 4, tmp_path / "missing")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    assert _bce("-gk", 4, empty).returncode == 255 and _bce("-gkd", 4, empty).returncode == 254
    r = _bce("-gkd", 4, src)                                             # not an archive: -gd's answer
    assert r.returncode == _bce("-gd", "abra", src).returncode != 0 and "k-grams" not in r.stdout
    r = _bce("-gk", 1, src)
    assert r.returncode == 0 and "\n1 5 0 500 " in r.stdout and r.stdout.endswith("1100 bytes\n")
