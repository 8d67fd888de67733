"""GPU: `bce -ge[i] EXPR file`, `-ge[i]d EXPR archive`, `-ge[i]l` and `-ge[i]ld` -- what a sliding window over the bytes finds for an
expression of byte classes: the count, or the byte offsets in ascending order and the count; from the index K1 and K2 build on the
GPU; nothing is written.  Compared line for line with Python's `re` on the same bytes, for expressions both understand (every
start of a match counts: a lookahead), and with tests/class_ref.py; a search beyond the default budget gives up and says so."""
import os
import re
import subprocess

import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import class_ref as ref

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
BANNER_LINES = 4                                                         # three lines and a blank one


def _bce(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _listing(d):
    return sorted((p.name, p.stat().st_size, p.stat().st_mtime_ns) for p in d.iterdir())


def test_the_commands_on_a_file_an_archive_and_a_checked_container(tmp_path):
    data = bce_amd.synth_text(23, 4000).tobytes()
    src, arc, blob = tmp_path / "in.txt", tmp_path / "a.bce", tmp_path / "a.bcem"
    src.write_bytes(data)
    assert _bce("-c", arc, src).returncode == 0 and _bce("-C3", blob, src).returncode == 0
    before = _listing(tmp_path)
    banner = _bce("-g", "the", src).stdout.split("\n")[:BANNER_LINES]
    assert banner[0] == "BCE v0.4 Release" and banner[-1] == ""
    seen = 0
    for expr, cases, archives in (("t[aeiou]e", (False,), True), ("T[AEIOU]e", (True,), True), ("[a-f][a-z]{2} ", (False,), False), ("[^a-z ]", (False, True), False),
                                  ("\\x74h.", (False,), False), ("e{2}", (True,), False)):
        for ignore_case in cases:
            rx = re.compile(b"(?=(" + expr.encode() + b"))", re.DOTALL | (re.IGNORECASE if ignore_case else 0))
            want = [m.start() for m in rx.finditer(data)]
            assert want == ref.hits(data, api.compile_classes(expr, ignore_case=ignore_case), cyclic=False).tolist()
            seen += len(want)
            tail = ["%d occurrences" % len(want), ""]
            want_c, want_l = "\n".join(banner + tail), "\n".join(banner + ["%d" % p for p in want] + tail)
            i = "i" if ignore_case else ""
            for files in ((src, ""), (arc, "d"), (blob, "d"))[:3 if archives else 1]:
                r = _bce("-ge" + i + files[1], expr, files[0])
                assert r.returncode == 0 and r.stdout == want_c, (expr, files, r.stdout + r.stderr)
                r = _bce("-ge" + i + "l" + files[1], expr, files[0])
                assert r.returncode == 0 and r.stdout == want_l, (expr, files, r.stdout + r.stderr)
    assert seen > 100
    # the last bytes and the first, with one byte free in between: a hit of the circular text only
    across = "".join("\\x%02x" % c for c in data[-3:]) + "." + "".join("\\x%02x" % c for c in data[1:3])
    assert ref.count(data, api.compile_classes(across)) >= 1 and ref.count(data, api.compile_classes(across), cyclic=False) == 0
    assert _bce("-ge", across, src).stdout == "\n".join(banner + ["0 occurrences", ""]) == _bce("-gel", across, src).stdout
    r = _bce("-ge", "a{4096}", src)                                      # fewer bytes than classes: nowhere
    assert r.returncode == 0 and r.stdout == "\n".join(banner + ["0 occurrences", ""])
    r = _bce("-ge", ".{65}", src)                                        # more sets of two bytes or more than the search has frames
    assert r.returncode == 252 and "Count failed" in r.stdout and "more than 64" in r.stdout and "occurrences" not in r.stdout
    assert _bce("-ge", "the", src).stdout == _bce("-g", "the", src).stdout and _bce("-gel", "the", src).stdout == _bce("-gl", "the", src).stdout
    assert _listing(tmp_path) == before


def test_a_search_beyond_the_budget_gives_up_and_says_so(tmp_path):
    """2 MiB of random bytes hold far more different strings of one, two and three bytes than the budget has nodes: `.{3}` ends at it."""
    data = bce_amd.synth_rand(5, 1 << 21).tobytes()
    src = tmp_path / "rand.bin"
    src.write_bytes(data)
    line = "search gave up: more than %d partial matches" % api.CLASS_DEFAULT_NODES
    banner = _bce("-g", "a", src).stdout.split("\n")[:BANNER_LINES]
    for cmd in ("-ge", "-gel"):
        r = _bce(cmd, ".{3}", src)
        assert r.returncode == 1 and r.stdout == "\n".join(banner + [line, ""]), r.stdout[-300:] + r.stderr
    want = sum(1 for a, b in zip(data, data[1:]) if a < 64 and b >= 128)
    r = _bce("-ge", "[\\x00-\\x3f][\\x80-\\xff]", src)                    # 128 + 64 * 128 nodes: within it
    assert r.returncode == 0 and r.stdout == "\n".join(banner + ["%d occurrences" % want, ""]) and want > 100000


def test_missing_inputs_give_the_existing_error_exits(tmp_path):
    for cmd in ("-ge", "-gei", "-gel"):
        r = _bce(cmd, "a[bc]", tmp_path / "missing")
        assert r.returncode == 255 and "Error loading file" in r.stdout and "occurrences" not in r.stdout
        r = _bce(cmd + "d", "a[bc]", tmp_path / "missing")
        assert r.returncode == 255 and "Archive not found." in r.stdout
