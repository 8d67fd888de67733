"""CPU: the rules the self-index kernels share with the host (bce_amd/csrc/lpf_step.h) compiled by g++ into a stand-alone program
under ASan + UBSan and driven through the kernels' block decomposition with blocks of 4 and 8 rows (tests/lpf_emul.cpp), against
the definitions in tests/lpf_ref.py: all nearest smaller values, the longest previous factor by brute force in ROTATION order with
tied rotations shuffled, every source by content and order, the chain, info, the sequential decoder, and that the parse with
min_len 1 has the fewest phrases (a dynamic programme); the new symbols and names; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import bce_amd
from bce_amd import api
from conftest import ROOT

import lpf_ref as ref
from test_count_cpu import _texts

SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
BOUNDS = (1, 3, 7, 4096)
MIN_LENS = (1, 3, 8)
NONE = ref.NONE
TAIL_REPEATS_HEAD = [b"abab", b"abcXabc", b"abcabcab", b"aXa", b"abcdefgh" * 3 + b"abcd", b"xyxyxyxyx"]   # the cyclic match runs past n - i


def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "lpf_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "lpf_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _words(v):
    return ",".join(str(int(x)) for x in v) or "-"


def _unwords(s):
    return [] if s == "-" else [int(x) for x in s.split(",")]


def _run(emul, tmp_path, lines):
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _self(line):
    w = line.split(" ")
    assert w[0] == "self" and len(w) == 9, line
    ops = np.array([] if w[3] == "-" else [[int(x) for x in p.split(":")] for p in w[3].split(",")], dtype=np.uint32).reshape(-1, 2)
    lits = b"" if w[4] == "-" else bytes.fromhex(w[4])
    return _unwords(w[1]), _unwords(w[2]), ops, lits, dict(zip(("nops", "nlits", "ncopies", "copied"), map(int, w[5:9])))


def _all_texts():
    texts, rs = _texts()
    assert len(texts) == 57
    periodic = [b"ab" * 9, b"abc" * 7, b"a" * 19, b"abcab" * 4, b"\x00\x01" * 12, b"aab" * 6]
    return texts + periodic + TAIL_REPEATS_HEAD, len(texts), rs


def test_nearest_smaller_values_in_blocks_of_4_and_8(tmp_path):
    emul = _build_emul()
    rs = np.random.RandomState(1808)
    arrays = [[5], [1, 2], [2, 1], [7] * 9, list(range(20)), list(range(20, 0, -1)), [3, 3, 1, 1, 2, 2, 1, 1, 3, 3, 0, 0, 4],
              [0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF] * 3]
    for m in (1, 2, 4, 5, 8, 13):                                            # the mountain: every far distance once on each side
        arrays.append([2 * p + 1 for p in range(m)] + [2 * (m - 1 - p) for p in range(m)])
    for k in range(150):
        n = int(rs.randint(1, 70))
        arrays.append(rs.permutation(n).tolist() if k % 2 else rs.randint(0, 1 + k % 5, n).tolist())
    lines = ["nsv %d %s" % (B, _words(a)) for a in arrays for B in (4, 8)]
    out = _run(emul, tmp_path, lines)
    far = 0
    for k, a in enumerate(arrays):
        psv, nsv = ref.ansv(a)
        for j, B in enumerate((4, 8)):
            w = out[2 * k + j].split(" ")
            assert w[0] == "nsv" and _unwords(w[1]) == psv.tolist() and _unwords(w[2]) == nsv.tolist(), (a, B)
        far += sum(1 for r, p in enumerate(psv.tolist() + nsv.tolist()) if p != NONE and abs(p // 4 - r % len(a) // 4) > 1)
    assert far > 100                                                         # answers further away than the neighbouring block
    m = 13
    psv, nsv = ref.ansv(arrays[8 + 5])
    assert psv.tolist() == [p - 1 if p else NONE for p in range(m)] + [m - 2 - p if p < m - 1 else NONE for p in range(m)]
    assert nsv.tolist() == [2 * m - 1 - p for p in range(m)] + [m + p + 1 if p < m - 1 else NONE for p in range(m)]
    assert all((a == NONE).all() for a in ref.ansv([4, 4, 4]))           # strict: an equal value is not smaller


def test_lpf_and_chain_in_rotation_order_against_brute_force(tmp_path):
    emul = _build_emul()
    texts, nplain, rs = _all_texts()
    cases, lines = [], []
    for k, t in enumerate(texts):
        orders = [ref.rotation_order(t)] + ([ref.rotation_order(t, rs) for _ in range(3)] if k >= nplain or len(set(t)) < 3 else [])
        for sa in orders:
            for m in MIN_LENS:
                for L in (L for L in BOUNDS if L >= m):
                    for B in (4, 8):
                        cases.append((t, m, L))
                        lines.append("self %d %d %d %s %s" % (B, m, L, _hex(t), _words(sa)))
    assert len(cases) > 2000
    brute, crossing, truncated = {}, 0, 0
    for (t, m, L), line in zip(cases, _run(emul, tmp_path, lines)):
        lpf, src, ops, lits, info = _self(line)
        if (t, L) not in brute:
            brute[t, L] = ref.lpf_brute(t, L)
            assert ref.lpf(t, L) == brute[t, L]                              # the reference the GPU tests use on larger texts
        assert lpf == brute[t, L], (t, L)
        ref.check_src(t, lpf, src)
        want = ref.chain(brute[t, L], t, m)
        ref.check(t, want, ops, lits, info)
        assert ref.decode(ops, lits) == t                                    # without the text
        assert info["nops"] - info["ncopies"] == sum(1 for p in want[0] if not p[2])
        if m == 1:
            assert info["ncopies"] + info["nlits"] == ref.fewest_phrases(t, L), (t, L)
        crossing += any(ln > 8 for _s, ln, _c in want[0])
        truncated += any(l == len(t) - i and l < L for i, l in enumerate(lpf) if l)
    assert crossing > 100 and truncated > 100                                # jumps across blocks; factors that end with the text
    assert ref.lpf_brute(b"abab", 4096) == [0, 0, 2, 1] and ref.lpf_brute(b"abcXabc", 4096) == [0, 0, 0, 0, 3, 2, 1]
    assert ref.lpf_brute(b"aaaa", 4096) == [0, 3, 2, 1] and ref.lpf_brute(b"aaaa", 2) == [0, 2, 2, 1]
    assert ref.self_parse(b"abracadabra", 1, 4096)[0] == [(0, 3, False), (3, 1, True), (4, 1, False), (5, 1, True), (6, 1, False), (7, 4, True)]
    assert ref.decode(np.array([[1, NONE], [5, 0]], dtype=np.uint32), b"a") == b"aaaaaa"        # a copy that overlaps its own output


def test_min_len_1_has_the_fewest_phrases_on_random_texts(tmp_path):
    emul = _build_emul()
    rs = np.random.RandomState(20260218)
    cases, lines = [], []
    for k in range(300):
        sigma = 2 + k % 3
        t = bytes(rs.randint(97, 97 + sigma, size=rs.randint(1, 28)).astype(np.uint8)) if k % 4 else bytes(rs.randint(97, 99, size=rs.randint(1, 4)).astype(np.uint8)) * int(rs.randint(2, 7))
        for L in (1, 2, 3, 5, 4096):
            cases.append((t, L))
            lines.append("self %d 1 %d %s %s" % (4 + 4 * (k % 2), L, _hex(t), _words(ref.rotation_order(t, rs))))
    for (t, L), line in zip(cases, _run(emul, tmp_path, lines)):
        lpf, _src, ops, lits, info = _self(line)
        assert lpf == ref.lpf_brute(t, L), (t, L)
        assert ref.decode(ops, lits) == t
        assert info["ncopies"] + info["nlits"] == ref.fewest_phrases(t, L), (t, L)
    assert ref.fewest_phrases(b"abcabcabc", 4096) == 4 and ref.fewest_phrases(b"abcabcabc", 2) == 6


def test_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("nsv 5 1,2\n", "nsv 4 -\n", "self 4 0 1 61 0\n", "self 4 2 1 61 0\n", "self 4 1 1 6161 0\n", "self 4 1 1 6161 0,2\n", "what 4 1\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


# ---- ABI, names -------------------------------------------------------------------------------------------------------------------

NEW = {"bce_hip_lpf": 4, "bce_hip_lpf_device": 4, "bce_hip_self_parse": 8, "bce_hip_self_parse_device": 8, "bce_hip_nsv_device": 5,
       "bce_hip_self_parse_of_lpf_device": 11}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert src.index("bce_hip_parse_of_lengths_device(") < src.index("bce_hip_lpf(") < src.index("bce_hip_sort_pairs_device(")   # a section of its own after the delta's
    whole = open(os.path.join(ROOT, "include", "bce_hip.h")).read()
    assert "A linear variant is out of scope" not in whole and "bce_hip_lpf" in whole[whole.index("by ITSELF"):whole.index("int bce_hip_lcp(")]
    for name in ("lpf", "self_parse", "lpf_tensor", "self_parse_tensor", "self_parse_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("lpf", "lpf_device", "self_parse", "self_parse_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name
        assert inspect.signature(getattr(bce_amd.RankFile, name)).parameters["max_len"].default == api.PARSE_MAX_LEN
    assert callable(api.nsv_device) and callable(api.self_parse_of_lpf_device)
    assert inspect.signature(bce_amd.lpf).parameters["max_len"].default == api.PARSE_MAX_LEN
    assert inspect.signature(bce_amd.self_parse).parameters["max_len"].default == api.PARSE_MAX_LEN


def test_null_context_is_refused_and_leaves_the_outputs_untouched():
    lib = bce_amd.load_library()
    words, more = (C.c_uint32 * 4)(7, 7, 7, 7), (C.c_uint32 * 4)(8, 8, 8, 8)
    lits, info = (C.c_uint8 * 4)(9, 9, 9, 9), api.ParseInfo(1, 2, 3, 4)
    for fn in (lib.bce_hip_lpf, lib.bce_hip_lpf_device):
        assert fn(None, 16, C.addressof(words), C.addressof(more)) == -1
        assert fn(None, 0, None, None) == -1
    for fn in (lib.bce_hip_self_parse, lib.bce_hip_self_parse_device):
        assert fn(None, 1, 16, C.addressof(words), 2, C.addressof(lits), 4, C.byref(info)) == -1
        assert fn(None, 1, 16, None, 0, None, 0, None) == -1
    assert lib.bce_hip_nsv_device(None, C.addressof(words), 4, C.addressof(more), C.addressof(more)) == -1
    assert lib.bce_hip_self_parse_of_lpf_device(None, None, None, None, 0, 1, None, 0, None, 0, C.byref(info)) == -1
    assert list(words) == [7] * 4 and list(more) == [8] * 4 and list(lits) == [9] * 4
    assert (info.nops, info.nlits, info.ncopies, info.copied) == (1, 2, 3, 4)


# ---- the command line without a device ----------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")


def _cli(tmp_path, *args):
    """(first line behind the banner and its blank line, exit status) of `bce args`, run in an empty directory"""
    work = tmp_path / "work"
    work.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, cwd=str(work))
    assert os.listdir(str(work)) == [], args
    lines = r.stdout.split("\n")
    return lines[lines.index("") + 1], r.returncode


def test_cli_bad_bounds_end_in_the_usage_text_and_files_are_judged_before_the_device(tmp_path):
    text, empty, missing = tmp_path / "text", tmp_path / "empty", tmp_path / "missing"
    text.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    for args in (("-gz",), ("-gz", 4), ("-gz", 4, text, "x"), ("-gz", 0, text), ("-gz", 4097, text), ("-gz", "4x", text), ("-gz", "", text),
                 ("-gz", "+4", text), ("-gz", " 4", text), ("-gz", -1, text), ("-gz", "4.0", text), ("-gz", 99999999999, text), ("-gzx", 4, text),
                 ("-gzd", 4), ("-gzd", 0, text), ("-gzd", 4097, text), ("-gzd", 4, text, "x")):
        assert _cli(tmp_path, *args) == ("Usage:", 0), args
    for m in (1, 16, 4096):                                                  # -gm's answers and exit codes
        for indexed in (missing, empty):
            assert _cli(tmp_path, "-gz", m, indexed) == ("Error loading file", 255)
        assert _cli(tmp_path, "-gzd", m, missing) == ("Archive not found.", 255)
        assert _cli(tmp_path, "-gzd", m, empty) == ("Could not read Archive.", 254)


def test_usage_has_the_two_paragraphs_behind_the_count_lines():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gd PATTERN archive.bce")
    assert lines[at + 2] == "" and lines[at + 3] == "  bce -gz MINLEN file" and lines[at + 4].startswith("   ") and "1..4096" in lines[at + 4]
    assert lines[at + 5] == "" and lines[at + 6] == "  bce -gzd MINLEN archive.bce" and lines[at + 7].startswith("   ")
    assert lines[at + 8] == "" and lines[at + 9] == "  bce -gl PATTERN file"
