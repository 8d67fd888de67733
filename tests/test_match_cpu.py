"""CPU: the lines the match kernel shares with the host (bce_amd/csrc/fm_step.h: fm_match_end) compiled by g++ into a stand-alone
program under ASan + UBSan, on planes built naively from a BWT and a suffix array made in Python, against a brute-force scan of the
text: the lengths in both modes for every bound, every position checked, the coverage; the new symbols, names and usage lines, and
the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bce_amd
from bce_amd import api
from conftest import ROOT

import locate_ref
import match_ref as ref
from test_count_cpu import _texts

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
BOUNDS, MIN_LENS = (1, 2, 7, 4096), (1, 3, 8)


def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "match_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "match_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _queries_for(text, rs):
    """The text itself; the text rotated; the text with single bytes changed; bytes the text lacks; and a query longer than the
    text that goes round it more than twice (on a periodic text the cyclic match is longer than n)."""
    n = len(text)
    cut = int(rs.randint(0, n))
    changed = bytearray(text * 2)
    for at in sorted({0, n // 2, n - 1, n + cut}):
        changed[at] ^= 1 + int(rs.randint(0, 255))
    qs = [text, text[cut:] + text[:cut], bytes(changed), (text * 3)[cut:cut + 2 * n + 3]]
    absent = [v for v in range(256) if v not in set(text)][:2]
    if absent:
        qs += [bytes(absent) * 3, text[:3] + bytes(absent[:1]) + text[-3:] + text[:2]]
    return qs


def _case(text, qs, sa=None):
    text = bytes(text)
    sa = locate_ref.suffix_array_of_rotations(text) if sa is None else sa
    bwt = bytes(text[(i - 1) % len(text)] for i in sa)
    return "%d %d\n%s\n%s\n%s\n" % (len(text), len(qs), _hex(bwt), " ".join(map(str, sa)), "\n".join(_hex(q) for q in qs))


def _words(field):
    return np.array([] if field == "-" else [int(v) for v in field.split(",")], dtype=np.uint32)


def _parse(stdout):
    """-> per case {(kind, mode, parameter): [one entry per query]}, the queries in input order"""
    cases = []
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cases.append({})
        elif w[0] == "m":
            cases[-1].setdefault(("m", w[1], int(w[2])), []).append((_words(w[3]), _words(w[4])))
        else:
            assert w[0] == "v", line
            cases[-1].setdefault(("v", w[1], int(w[2])), []).append(int(w[3]))
    return cases


def test_lengths_positions_and_coverage_are_the_brute_force_ones(tmp_path):
    emul = _build_emul()
    texts, rs = _texts()
    assert len(texts) == 57
    # tied rotations of a periodic text may stand in any order: the same answers from the reversed ties
    extra = [(b"abab", [2, 0, 3, 1]), (b"aaaa", [3, 1, 0, 2]), (b"\x00\xff" * 5, [8, 6, 4, 2, 0, 9, 7, 5, 3, 1])]
    cases = [(t, _queries_for(t, rs), None) for t in texts] + [(t, _queries_for(t, rs), sa) for t, sa in extra]
    src = tmp_path / "cases.txt"
    src.write_text("".join(_case(t, qs, sa) for t, qs, sa in cases))
    want = {}
    differ = 0
    for t, qs, _ in cases:
        for q in qs:
            for cyclic in (True, False):
                for L in sorted(set(BOUNDS + MIN_LENS)):
                    want[(t, q, cyclic, L)] = ref.match_lens(t, q, L, cyclic)
            differ += not np.array_equal(want[(t, q, True, 4096)], want[(t, q, False, 4096)])
    assert differ > 100                                                   # matches across the end of the text: the modes disagree
    for from_stdin in (False, True):                                      # a file, and stdin
        with open(src) as f:
            r = subprocess.run([emul] if from_stdin else [emul, str(src)], stdin=f if from_stdin else None, capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        got = _parse(r.stdout)
        assert len(got) == len(cases)
        for (t, qs, _), g in zip(cases, got):
            for mode, cyclic in (("c", True), ("l", False)):
                for L in BOUNDS:
                    assert len(g[("m", mode, L)]) == len(qs)
                    for q, (lens, pos) in zip(qs, g[("m", mode, L)]):
                        assert np.array_equal(lens, want[(t, q, cyclic, L)]), (t, q, mode, L)
                        ref.check_positions(t, q, lens, pos, cyclic)
                        assert (lens[1:].astype(np.int64) <= lens[:-1].astype(np.int64) + 1).all() and int(lens.max()) <= L
                for m in MIN_LENS:
                    for q, cov in zip(qs, g[("v", mode, m)]):
                        assert cov == ref.covered(want[(t, q, cyclic, m)], m), (t, q, mode, m)
                        assert cov == ref.covered(want[(t, q, cyclic, 4096)], m)   # a bound of min_len is enough
    # what the cases cover
    assert ref.match_lens(b"abab", b"ab" * 5, 4096, True).tolist() == list(range(1, 11))           # longer than n, cyclic
    assert ref.match_lens(b"abab", b"ab" * 5, 4096).tolist() == [1, 2, 3, 4, 3, 4, 3, 4, 3, 4]
    assert ref.match_lens(b"abracadabra", b"raab", 4096, True).tolist() == [1, 2, 3, 4]            # across the end
    assert ref.match_lens(b"abracadabra", b"raab", 4096).tolist() == [1, 2, 1, 2]
    assert ref.match_lens(b"abracadabra", b"abrxcad", 3).tolist() == [1, 2, 3, 0, 1, 2, 3]         # cut short at the bound
    assert ref.covered(np.array([1, 2, 3, 0, 1, 2, 3]), 3) == 6 and ref.covered(np.array([1, 2, 3, 0, 1, 2, 3]), 4) == 0
    assert ref.covered(np.array([0, 0, 3, 0, 1]), 2) == 3 and ref.covered(np.array([0, 1, 0, 0]), 1) == 1


def test_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("3 1\n6162\n0 1 2\n61\n", "2 1\n6261\n0 0\n61\n", "2 1\n6261\n0 2\n61\n", "2 2\n6261\n0 1\n61\n", "0 0\n-\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_match": 7, "bce_hip_match_device": 7, "bce_hip_coverage": 6, "bce_hip_coverage_device": 6}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"#define\s+BCE_HIP_MATCH_LINEAR\s+1u", src) and api.MATCH_LINEAR == 1
    for name in ("match", "coverage", "match_tensor", "coverage_tensor", "coverage_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    assert callable(bce_amd.RankFile.match) and callable(bce_amd.RankFile.match_device) and callable(bce_amd.RankFile.coverage)


def test_null_context_and_refused_arguments_leave_the_outputs_untouched():
    lib = bce_amd.load_library()
    qry = (C.c_uint8 * 4)(97, 98, 99, 100)
    lens, pos, cov = (C.c_uint32 * 4)(7, 7, 7, 7), (C.c_uint32 * 4)(9, 9, 9, 9), C.c_uint64(5)
    for fn in (lib.bce_hip_match, lib.bce_hip_match_device):
        assert fn(None, C.addressof(qry), 4, 16, 1, C.addressof(lens), C.addressof(pos)) == -1
        assert fn(None, None, 0, 16, 0, None, None) == -1
    for fn in (lib.bce_hip_coverage, lib.bce_hip_coverage_device):
        assert fn(None, C.addressof(qry), 4, 16, 1, C.byref(cov)) == -1
        assert fn(None, None, 0, 16, 0, C.byref(cov)) == -1
    assert list(lens) == [7] * 4 and list(pos) == [9] * 4 and cov.value == 5


def test_usage_has_the_two_match_lines_directly_after_the_locate_lines():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gld PATTERN archive.bce")
    assert lines[at + 2] == "" and lines[at + 3] == "  bce -gm MINLEN file query_file"
    assert lines[at + 5] == "" and lines[at + 6] == "  bce -gmd MINLEN archive.bce query_file"
    for args in (["-gm"], ["-gm", "16"], ["-gm", "16", "file"], ["-gm", "0", "file", "query"], ["-gm", "4097", "file", "query"],
                 ["-gm", "16x", "file", "query"], ["-gm", "", "file", "query"], ["-gmx", "16", "file", "query"],
                 ["-gmd", "16", "a", "b", "c"]):                        # no command: the usage text
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_match_without_a_device_answers_as_the_count_does(tmp_path):
    """The CLI as tests/test_count_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the coverage's
    entry point is a weak reference and stays unresolved.  Both files are read and judged before the device is missed, with -g's
    words and exit codes."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_match")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f, qf, empty, missing = tmp_path / "in.txt", tmp_path / "query.txt", tmp_path / "empty", tmp_path / "missing"
    f.write_bytes(b"abracadabra" * 100)
    qf.write_bytes(b"cadabra abra")
    empty.write_bytes(b"")
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, cwd=tmp_path)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        return r

    for dflag in ("", "d"):
        for file in (missing, empty, f):                                 # the indexed file: -g's answer
            a, b = run("-g" + dflag, "abra", file), run("-gm" + dflag, 4, file, qf)
            assert a.returncode == b.returncode != 0 and a.stdout == b.stdout, (file, dflag, b.stdout)
        for query in (missing, empty):                                   # the query is a plain file in both commands: -g's words for one
            a, b = run("-g", "abra", query), run("-gm" + dflag, 4, f, query)
            assert a.returncode == b.returncode == 255 and a.stdout == b.stdout and "Error loading file" in b.stdout, (query, dflag)
    r = run("-gm", 4, f, qf)
    assert r.returncode == 253 and "No usable HIP device" in r.stdout
    assert sorted(os.listdir(tmp_path)) == before
