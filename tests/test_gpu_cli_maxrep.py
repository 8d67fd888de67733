"""GPU: `bce -gp ORDER MINLEN N file` and `bce -gpd ORDER MINLEN N archive` -- a head line, then the N heaviest maximal repeats of the
circular text as `LEN COUNT POS ESCAPED`, then the closing line: length, count and bytes line for line what Python formats from
tests/maxrep_ref.py, the position checked (its cyclic cut is the repeat); nothing is written."""
import os
import subprocess

import pytest

import bce_amd
from conftest import ROOT

import count_ref
import maxrep_ref as ref
import top_ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
BANNER_LINES = 4                                                         # three lines and a blank one
BOUND, SHOWN = 4096, 64


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def _check(data, order, min_len, N, stdout, banner=None):
    lines = stdout.split("\n")
    if banner is not None:
        assert lines[:BANNER_LINES] == banner
    want, info = ref.of_text(data, min_len, BOUND, order, N)
    body = lines[BANNER_LINES:]
    assert body[0] == "maximal repeats of the circular text by %s: length count position bytes" % order
    last = "%d maximal repeats of %d bytes or more (%d of 4096 or more), %d BWT runs, %d bytes" % (info["total"], min_len, info["capped"], info["bwt_runs"], len(data))
    assert len(body) == len(want) + 3 and body[-2:] == [last, ""], stdout[-400:]
    for line, (length, count, _) in zip(body[1:], want):
        w = line.split(" ")
        assert len(w) == 4 and w[0] == ("%d+" % length if length == BOUND else str(length)) and w[1] == str(count), (line, length, count)
        cut = count_ref.cyclic_cut(data, int(w[2]), min(length, SHOWN))
        assert 0 <= int(w[2]) < len(data) and w[3] == top_ref.escape(cut) + ("..." if length > SHOWN else ""), line
    return want, info


def test_the_list_of_a_file_an_archive_and_both_container_kinds(tmp_path):
    data = bce_amd.synth_text(23, 9000).tobytes()
    src, arc, blob, plain = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem", tmp_path / "b.bcem"
    src.write_bytes(data)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C2", blob, src).returncode == 0 and _bce("-c2", plain, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "the", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    for order, min_len, N in (("len", 1, 10), ("count", 3, 65536), ("gain", 2, 7), ("len", 4096, 3)):
        for args in (("-gp", order, min_len, N, src), ("-gpd", order, min_len, N, arc), ("-gpd", order, min_len, N, blob), ("-gpd", order, min_len, N, plain)):
            r = _bce(*args)
            assert r.returncode == 0, (args, r.stdout + r.stderr)
            _check(data, order, min_len, N, r.stdout, banner)
    assert _listing(tmp_path) == before


def test_repeats_at_the_bound_escaped_bytes_and_texts_without_repeats(tmp_path):
    block = bce_amd.synth_rand(22, 5000).tobytes()
    cases = {"periodic": b"ab" * 150, "one": b"z", "abra": b"abracadabra", "blank": b"a b\\c\n" * 20 + b"\x00\xff\x7f",
             "paste": bce_amd.synth_rand(21, 3000).tobytes() + block + b"\x00 \\" + block}
    for name, data in cases.items():
        f = tmp_path / name
        f.write_bytes(data)
        for order, min_len, N in (("len", 1, 300), ("gain", 2, 5), ("count", 1, 65536)):
            r = _bce("-gp", order, min_len, N, f)
            assert r.returncode == 0, r.stdout + r.stderr
            _check(data, order, min_len, N, r.stdout)
    body = _bce("-gp", "len", 1, 9, tmp_path / "abra").stdout.split("\n")[BANNER_LINES:]
    assert [line.split(" ")[::3] for line in body[1:3]] == [["4", "abra"], ["1", "a"]] and [line.split(" ")[1] for line in body[1:3]] == ["2", "5"]
    assert body[3] == "2 maximal repeats of 1 bytes or more (0 of 4096 or more), 7 BWT runs, 11 bytes"
    for name, runs, n in (("periodic", 2, 300), ("one", 1, 1)):
        assert _bce("-gp", "len", 1, 9, tmp_path / name).stdout.split("\n")[BANNER_LINES + 1] == "0 maximal repeats of 1 bytes or more (0 of 4096 or more), %d BWT runs, %d bytes" % (runs, n)
    first = _bce("-gp", "len", 1, 1, tmp_path / "paste").stdout.split("\n")[BANNER_LINES + 1].split(" ")
    assert first[:2] == ["4096+", "2"] and first[3].endswith("...")


def test_missing_and_empty_inputs_give_the_count_commands_exits(tmp_path):
    src, empty = tmp_path / "in.txt", tmp_path / "empty"
    src.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    r = _bce("-gp", "len", 4, 5, tmp_path / "missing")
    assert r.returncode == 255 and "Error loading file" in r.stdout and "maximal repeats" not in r.stdout
    r = _bce("-gpd", "len", 4, 5, tmp_path / "missing")
    assert r.returncode == 255 and "Archive not found." in r.stdout
    assert _bce("-gp", "len", 4, 5, empty).returncode == 255 and _bce("-gpd", "len", 4, 5, empty).returncode == 254
    r = _bce("-gpd", "len", 4, 5, src)                                    # not an archive: -gd's answer
    assert r.returncode == _bce("-gd", "abra", src).returncode != 0 and "maximal repeats" not in r.stdout
