"""CPU: the lines the locate kernels share with the host (bce_amd/csrc/fm_step.h: fm_range, the row-to-pattern search, the linear
filter) compiled by g++ into a stand-alone program under ASan + UBSan, on planes built naively from a BWT and a suffix array made
in Python, against a brute-force scan of the text; the new symbols, names and usage lines, and the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import bce_amd
from bce_amd import api
from conftest import ROOT

import count_ref
import locate_ref as ref
from test_count_cpu import _patterns_for, _texts

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "locate_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "locate_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _case(text, pats, sa=None):
    text = bytes(text)
    sa = ref.suffix_array_of_rotations(text) if sa is None else sa
    bwt = bytes(text[(i - 1) % len(text)] for i in sa)
    return "%d %d\n%s\n%s\n%s\n" % (len(text), len(pats), _hex(bwt), " ".join(map(str, sa)), "\n".join(_hex(p) for p in pats))


def _parse(stdout):
    cases = []
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cases.append([])
        else:
            assert w[0] == "c" and w[2] == "l", line
            cases[-1].append(tuple([] if h == "-" else [int(v) for v in h.split(",")] for h in (w[1], w[3])))
    return cases


def test_rows_of_the_suffix_array_are_the_brute_force_hits(tmp_path):
    emul = _build_emul()
    texts, rs = _texts()
    assert len(texts) == 57
    lines, want, all_pats = [], [], []
    for t in texts:
        pats = _patterns_for(t, rs)
        lines.append(_case(t, pats))
        all_pats.append(pats)
        want.append([(ref.cyclic_hits(t, p), ref.linear_hits(t, p) if p else []) for p in pats])
    # tied rotations of a periodic text may stand in any order: the same hits from the reversed ties
    extra = [(b"abab", [2, 0, 3, 1]), (b"aaaa", [3, 1, 0, 2]), (b"\x00\xff" * 5, [8, 6, 4, 2, 0, 9, 7, 5, 3, 1])]
    for t, sa in extra:
        pats = _patterns_for(t, rs)
        lines.append(_case(t, pats, sa))
        all_pats.append(pats)
        want.append([(ref.cyclic_hits(t, p), ref.linear_hits(t, p) if p else []) for p in pats])
    src = tmp_path / "cases.txt"
    src.write_text("".join(lines))
    for from_stdin in (False, True):                                                      # a file, and stdin
        with open(src) as f:
            r = subprocess.run([emul] if from_stdin else [emul, str(src)], stdin=f if from_stdin else None, capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        got = _parse(r.stdout)
        assert len(got) == len(want)
        for t, pats, g, w in zip(texts + [e[0] for e in extra], all_pats, got, want):
            assert len(g) == len(w)
            for p, (gc, gl), (wc, wl) in zip(pats, g, w):
                assert gc == wc, (t, p, "cyclic")
                assert len(gc) == count_ref.cyclic_count(t, p)
                if p:                                                 # (the empty pattern has no linear hits to ask for)
                    assert gl == wl, (t, p, "linear")
                    assert len(gl) == count_ref.linear_count(t, p)
    # what the cases cover: hits across the end dropped, every tied rotation of a periodic text, m > n, the empty pattern
    assert ref.cyclic_hits(b"abracadabra", b"aabr") == [10] and ref.linear_hits(b"abracadabra", b"aabr") == []
    assert ref.cyclic_hits(b"abab", b"ab" * 5) == [0, 2] and ref.linear_hits(b"abab", b"ab" * 5) == []
    assert ref.cyclic_hits(b"aaaa", b"aaa") == [0, 1, 2, 3] and ref.linear_hits(b"aaaa", b"aaa") == [0, 1]
    assert ref.cyclic_hits(b"abc", b"") == [0, 1, 2]


def test_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("3 1\n6162\n0 1 2\n61\n", "2 1\n6261\n0 0\n61\n", "2 1\n6261\n0 2\n61\n", "2 2\n6261\n0 1\n61\n", "0 0\n-\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_locate": 9, "bce_hip_locate_device": 9}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"#define\s+BCE_HIP_LOCATE_LINEAR\s+1u", src) and api.LOCATE_LINEAR == 1
    for name in ("locate", "locate_tensor", "locate_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    assert callable(bce_amd.RankFile.locate) and callable(bce_amd.RankFile.locate_device)


def test_null_context_and_total_are_refused_before_any_device_call():
    lib = bce_amd.load_library()
    pat, off = (C.c_uint8 * 4)(97, 98, 99, 100), (C.c_uint64 * 2)(0, 4)
    hits, pos, total = (C.c_uint64 * 2)(7, 7), (C.c_uint32 * 4)(9, 9, 9, 9), C.c_uint64(5)
    for fn in (lib.bce_hip_locate, lib.bce_hip_locate_device):
        assert fn(None, C.addressof(pat), C.addressof(off), 1, 1, C.addressof(hits), C.addressof(pos), 4, C.byref(total)) == -1
        assert fn(None, None, None, 0, 0, None, None, 0, C.byref(total)) == -1
    assert list(hits) == [7, 7] and list(pos) == [9] * 4 and total.value == 5


def test_usage_has_the_two_locate_lines_after_the_count_lines():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    out = r.stdout
    assert "  bce -gl PATTERN file\n" in out and "  bce -gld PATTERN archive.bce\n" in out
    assert out.index("  bce -gd PATTERN archive.bce\n") < out.index("  bce -gl PATTERN file\n") < out.index("  bce -gld PATTERN archive.bce\n")
    for args in (["-gl"], ["-gl", "abra"], ["-gl", "", "file"], ["-glx", "abra", "file"], ["-gld", "abra", "a", "b"]):   # no command: the usage text
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_locate_without_a_device_answers_as_the_count_does(tmp_path):
    """The CLI as tests/test_count_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the locate's entry
    point is a weak reference and stays unresolved.  Files are read and judged before the device is missed, with -g's words."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_locate")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f, empty = tmp_path / "in.txt", tmp_path / "empty"
    f.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    before = sorted(os.listdir(tmp_path))
    for file, dflag in ((f, ""), (tmp_path / "missing", ""), (empty, ""), (f, "d"), (tmp_path / "missing", "d"), (empty, "d")):
        ans = [subprocess.run([exe, flag + dflag, "abra", str(file)], capture_output=True, text=True, env=env, cwd=tmp_path) for flag in ("-g", "-gl")]
        for r in ans:
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        assert ans[0].returncode == ans[1].returncode != 0 and ans[0].stdout == ans[1].stdout, (file, dflag, ans[1].stdout)
    r = subprocess.run([exe, "-gl", "abra", str(f)], capture_output=True, text=True, env=env, cwd=tmp_path)
    assert r.returncode == 253 and "No usable HIP device" in r.stdout
    assert sorted(os.listdir(tmp_path)) == before
