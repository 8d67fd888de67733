"""CPU: backward search on the K2 planes (bce_amd/csrc/fm_step.h, the step kd_count.hip runs per pattern byte) compiled by g++
into a stand-alone program under ASan + UBSan, on planes built naively from a BWT made in Python, against a brute-force count
of the circular text; the seam correction that turns a cyclic count into a linear one against an overlapping scan; the new
symbols, names and usage lines, and the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import count_ref as ref

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def emul():
    exe = os.path.join(ROOT, "tests", "_build", "count_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "count_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _patterns_for(text, rs):
    """Cut from the circular text at every kind of place -- inside, across the end, as long as the text, longer -- plus patterns
    with a byte the text lacks, and the empty one."""
    n = len(text)
    pats = [b""]
    for m in sorted({1, 2, 3, n - 1, n, n + 1, 2 * n, 3 * n} - {0}):
        for start in sorted({0, n // 2, n - 1, int(rs.randint(0, n))}):
            pats.append(ref.cyclic_cut(text, start, m))
    absent = [v for v in range(256) if v not in set(text)][:2]
    for v in absent:
        pats += [bytes([v]), ref.cyclic_cut(text, 0, min(n, 3)) + bytes([v]), bytes([v]) + ref.cyclic_cut(text, n - 1, 2)]
    return pats


def _texts():
    rs = np.random.RandomState(96)
    texts = [b"a", b"ab", b"abab", b"aaaa", b"abracadabra", bytes(range(256)), b"\x00\xff" * 5]
    for i in range(50):
        sigma = (2, 3, 256)[i % 3]
        n = int(rs.randint(1, 41))
        texts.append(bytes(int(v) for v in rs.randint(0, sigma, n)))
    return texts, rs


def test_backward_search_on_naive_planes_is_the_brute_force_cyclic_count(emul, tmp_path):
    texts, rs = _texts()
    assert len(texts) == 57
    lines, want = [], []
    for t in texts:
        bwt, row0 = ref.bwt_of_rotations(t)
        pats = _patterns_for(t, rs)
        lines.append("%d %d %d\n%s\n%s\n" % (len(t), row0, len(pats), _hex(bwt), "\n".join(_hex(p) for p in pats)))
        want.append([ref.cyclic_count(t, p) for p in pats])
    src = tmp_path / "cases.txt"
    src.write_text("".join(lines))
    for how in ({"args": [emul, str(src)]}, {"args": [emul], "stdin": open(src)}):        # a file, and stdin
        r = subprocess.run(capture_output=True, text=True, env=SAN_ENV, **how)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        got = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
        assert len(got) == len(want)
        for t, g, w in zip(texts, got, want):
            assert g == w, t
    # what the cases cover: wrapped matches, periodic texts counted more than once per period, absent bytes, the empty pattern
    assert want[2][0] == 4 and ref.cyclic_count(b"abab", b"ab" * 5) == 2 and ref.cyclic_count(b"aaaa", b"a" * 12) == 4
    assert ref.cyclic_count(b"abracadabra", b"aabr") == 1 and ref.linear_count(b"abracadabra", b"aabr") == 0


def test_emulator_refuses_malformed_input(emul, tmp_path):
    for text in ("3 0 1\n6162\n61\n", "2 0 1\n616\n61\n", "2 0 2\n6162\n61\n", "0 0 0\n-\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


def test_seam_correction_turns_cyclic_counts_into_an_overlapping_scan():
    """linear = cyclic - matches in (last m - 1 bytes) + (first m - 1 bytes), for m <= n -- texts shorter than 2 (m - 1), where
    the two ends overlap, included; 0 for m > n."""
    texts, rs = _texts()
    short = 0
    for t in texts:
        n = len(t)
        pats = [p for p in _patterns_for(t, rs) if p]
        cyc = [ref.cyclic_count(t, p) for p in pats]
        got = api.linear_counts(cyc, pats, n, lambda k, t=t: (t[:k], t[len(t) - k:]))
        assert got.dtype == np.uint64
        for p, g in zip(pats, got):
            assert int(g) == ref.linear_count(t, p), (t, p)
            short += 1 < len(p) <= n < 2 * (len(p) - 1)
    assert short > 50
    assert api.seam_count(b"ab", b"xr", b"rab") == 1 and api.seam_count(b"", b"", b"a") == 0
    assert api.seam_count(b"aa", b"aa", b"aaa") == 2                 # text aaaa: 4 cyclic matches, 2 linear


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_count": 5, "bce_hip_count_device": 5, "bce_hip_input_bytes": 4}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    for name in ("count", "count_tensor", "count_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    assert callable(bce_amd.RankFile.count) and callable(bce_amd.RankFile.count_device)


def test_null_context_is_refused_before_any_device_call():
    lib = bce_amd.load_library()
    pat, off, out = (C.c_uint8 * 4)(97, 98, 99, 100), (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 1)(7)
    assert lib.bce_hip_count(None, C.addressof(pat), C.addressof(off), 1, C.addressof(out)) == -1
    assert lib.bce_hip_count_device(None, C.addressof(pat), C.addressof(off), 1, C.addressof(out)) == -1
    assert lib.bce_hip_count(None, None, None, 0, None) == -1
    assert lib.bce_hip_input_bytes(None, 0, 1, C.addressof(pat)) == -1
    assert out[0] == 7


def test_usage_has_the_two_count_lines_after_the_existing_ones():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    out = r.stdout
    assert "  bce -g PATTERN file\n" in out and "  bce -gd PATTERN archive.bce\n" in out
    assert out.index("  bce -e file [config.bcc]\n") < out.index("  bce -g PATTERN file\n") < out.index("  bce -gd PATTERN archive.bce\n")
    for args in (["-g"], ["-g", "abra"], ["-g", "", "file"], ["-gx", "abra", "file"], ["-gd", "abra", "a", "b"]):   # no command: the usage text
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_count_without_a_device_says_so(tmp_path):
    """The CLI as tests/test_checked_container_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the
    count's entry point is a weak reference and stays unresolved.  Files are read and judged before the device is missed."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_count")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f = tmp_path / "in.txt"
    f.write_bytes(b"abracadabra" * 100)
    before = sorted(os.listdir(tmp_path))
    for args, code, text in ((["-g", "abra", str(f)], 253, "No usable HIP device"), (["-gd", "abra", str(f)], 253, "No usable HIP device"),
                             (["-g", "abra", str(tmp_path / "missing")], 255, "Error loading file"),
                             (["-gd", "abra", str(tmp_path / "missing")], 255, "Archive not found.")):
        r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, cwd=tmp_path)
        assert r.returncode == code and text in r.stdout, (args, r.returncode, r.stdout)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == before
