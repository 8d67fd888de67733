"""CPU: the references of the LCP array and the k-gram classes checked against one another (tests/repeat_ref.py pins the yardstick
of tests/test_gpu_repeat.py); the compare the LCP kernel shares with the host (bce_amd/csrc/lcp_step.h: rot_lcp) compiled by g++
into a stand-alone program under ASan + UBSan, on texts in heap blocks of exactly n bytes; the new symbols, names and usage lines,
and the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bce_amd
from bce_amd import api
from conftest import ROOT

import locate_ref
import repeat_ref as ref
from test_count_cpu import _texts

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
BOUNDS = (1, 2, 7, 8, 9, 4096)
# tied rotations of a periodic text may stand in any order: the reversed ties tests/test_match_cpu.py uses
REVERSED_TIES = [(b"abab", [2, 0, 3, 1]), (b"aaaa", [3, 1, 0, 2]), (b"\x00\xff" * 5, [8, 6, 4, 2, 0, 9, 7, 5, 3, 1])]


def log2q(c):
    return api.cost_q24(1, c)


# ---- the references against one another ----------------------------------------------------------------------------------------------

def test_classes_from_the_capped_lcp_are_the_counted_kgrams():
    texts, _ = _texts()
    assert len(texts) == 57
    for t in texts:
        n = len(t)
        for k in (0, 1, 2, 3, 5, 8, n, n + 3):
            lcp = ref.capped_lcp(t, max(k, 1))
            assert ref.classes_of_lcp(lcp, k) == ref.kgram_classes(t, k), (t, k)
            assert sum(ref.kgram_classes(t, k)) == n
    assert ref.kgram_classes(b"abab", 7) == [2, 2] and ref.kgram_classes(b"aaaa", 9) == [4]            # k > n wraps around
    assert ref.kgram_classes(b"abracadabra", 2) == [1, 1, 1, 1, 1, 2, 2, 2]                            # "aa" across the end


def test_capped_lcp_is_the_compare_of_neighbouring_rotations_in_any_tie_order():
    texts, _ = _texts()
    for t in texts:
        sa = locate_ref.suffix_array_of_rotations(t)
        for L in BOUNDS:
            assert np.array_equal(ref.capped_lcp(t, L), ref.lcp_of_order(t, sa, L)), (t, L)
    for t, sa in REVERSED_TIES:
        assert sorted(sa) == list(range(len(t)))
        for L in BOUNDS:
            assert np.array_equal(ref.capped_lcp(t, L), ref.lcp_of_order(t, sa, L)), (t, L)
    assert ref.capped_lcp(b"aaaa", 4096).tolist() == [0, 4096, 4096, 4096]                             # no cap at n
    assert ref.capped_lcp(b"abab", 9).tolist() == [0, 9, 0, 9]
    assert ref.capped_lcp(b"abracadabra", 4096).tolist() == [0, 1, 4, 1, 1, 0, 3, 0, 0, 0, 2]


def test_entropy_from_the_q24_sums_is_the_float_definition():
    """|H_k from the integer sums - the float definition| <= 2^-20 bit: bce_cost.h states an error below 2^-21 bit per logarithm,
    and a class's share c * L(c) / n of S_k sums to at most that over the classes (their sizes add up to n) -- once in S_k and
    once in S_(k+1).  Derived, not measured."""
    texts, _ = _texts()
    worst = 0.0
    for t in texts:
        n = len(t)
        for k in (0, 1, 2, 3, 5, 8, n, n + 3):
            s = [ref.kgram_record(t, kk, log2q)[2] for kk in (k, k + 1)]
            h = ref.entropy_q24(n, s[0], s[1])
            assert h == bce_amd.entropy_from_sums(n, s[0], s[1])
            worst = max(worst, abs(h - ref.entropy_float(t, k)))
    print("largest difference: %.3g bit" % worst)
    assert worst <= 2.0 ** -20
    assert ref.kgram_record(b"abab", 1, log2q) == (2, 0, 2 * 2 * (1 << 24), 2)
    assert ref.kgram_record(b"a", 5, log2q) == (1, 1, 0, 1)


# ---- rot_lcp under the sanitizers ------------------------------------------------------------------------------------------------------

def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "lcp_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "lcp_emul.cpp")])
    return exe


def _case(text, sa=None):
    text = bytes(text)
    sa = locate_ref.suffix_array_of_rotations(text) if sa is None else sa
    return "%d\n%s\n%s\n" % (len(text), text.hex(), " ".join(map(str, sa)))


def test_rot_lcp_on_exactly_sized_heap_blocks_is_the_capped_lcp(tmp_path):
    emul = _build_emul()
    texts, rs = _texts()
    cases = [(t, None) for t in texts] + REVERSED_TIES
    for n in range(1, 18):                                               # every place of the wrap inside an eight-byte word
        cases.append((b"q" * n, None))
        cases.append((bytes(int(v) for v in rs.randint(0, 2, n)), None))
        cases.append((bytes(int(v) for v in rs.randint(0, 256, n)), None))
    cases.append((bytes(int(v) for v in rs.randint(0, 2, 300)), None))   # long agreements away from and across the seam
    cases.append((b"abcdefgh" * 9 + b"abcdefgx", None))
    src = tmp_path / "cases.txt"
    src.write_text("".join(_case(t, sa) for t, sa in cases))
    for from_stdin in (False, True):                                      # a file, and stdin
        with open(src) as f:
            r = subprocess.run([emul] if from_stdin else [emul, str(src)], stdin=f if from_stdin else None, capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases) * (1 + len(BOUNDS))
        for i, (t, _) in enumerate(cases):
            block = lines[i * (1 + len(BOUNDS)):(i + 1) * (1 + len(BOUNDS))]
            assert block[0] == "case %d" % len(t)
            for L, line in zip(BOUNDS, block[1:]):
                w = line.split()
                assert w[0] == "l" and int(w[1]) == L
                assert [int(v) for v in w[2].split(",")] == ref.capped_lcp(t, L).tolist(), (t, L)


def test_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("3\n6162\n0 1 2\n", "2\n6261\n0 0\n", "2\n6261\n0 2\n", "2\n6261\n0\n", "0\n\n", "2\n626\n0 1\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_lcp": 3, "bce_hip_lcp_device": 3, "bce_hip_kgrams": 4, "bce_hip_longest_repeat": 5}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    body = src[src.index("typedef struct bce_hip_kgram {"):src.index("} bce_hip_kgram;")]
    want = []
    for ctype, names in re.findall(r"\b(uint64_t|uint32_t)\s+([^;]+);", body):
        want += [(name.strip(), {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}[ctype]) for name in names.split(",")]
    assert [(n, t) for n, t in api.KGram._fields_] == want and C.sizeof(api.KGram) == 32
    assert re.search(r"#define\s+BCE_HIP_KGRAMS_MAX\s+64u", src) and api.KGRAMS_MAX == 64
    for name in ("kgrams", "entropy_profile", "longest_repeat", "lcp_tensor", "kgrams_tensor", "entropy_profile_tensor", "entropy_profile_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("lcp", "lcp_device", "kgrams", "entropy_profile", "longest_repeat"):
        assert callable(getattr(bce_amd.RankFile, name)), name


def test_null_context_and_refused_arguments_leave_the_outputs_untouched():
    lib = bce_amd.load_library()
    lcp = (C.c_uint32 * 4)(7, 7, 7, 7)
    ks = (C.c_uint32 * 3)(0, 1, 5000)
    recs = (api.KGram * 3)()
    for r in recs:
        r.distinct, r.max_pos = 11, 13
    ln, a, b = C.c_uint32(5), C.c_uint32(6), C.c_uint32(7)
    for max_len in (16, 0, 4097):
        assert lib.bce_hip_lcp(None, max_len, C.addressof(lcp)) == -1
        assert lib.bce_hip_lcp_device(None, max_len, C.addressof(lcp)) == -1
        assert lib.bce_hip_longest_repeat(None, max_len, C.byref(ln), C.byref(a), C.byref(b)) == -1
    for nk in (0, 2, 3, 65):
        assert lib.bce_hip_kgrams(None, C.addressof(ks), nk, C.addressof(recs)) == -1
    assert lib.bce_hip_kgrams(None, None, 0, None) == -1
    assert list(lcp) == [7] * 4 and (ln.value, a.value, b.value) == (5, 6, 7)
    assert all(r.distinct == 11 and r.max_pos == 13 for r in recs)


def test_usage_has_the_two_kgram_lines_directly_after_the_match_lines():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    at = lines.index("  bce -gmd MINLEN archive.bce query_file")
    assert lines[at + 2] == "" and lines[at + 3] == "  bce -gk K file"
    assert lines[at + 5] == "" and lines[at + 6] == "  bce -gkd K archive.bce"
    for args in (["-gk"], ["-gk", "4"], ["-gk", "33", "file"], ["-gk", "-1", "file"], ["-gk", "4x", "file"], ["-gk", "", "file"],
                 ["-gk", "+4", "file"], ["-gk", " 4", "file"], ["-gkx", "4", "file"], ["-gkd", "4", "a", "b"], ["-gkd", "4.0", "a"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_kgrams_without_a_device_answers_as_the_count_does(tmp_path):
    """The CLI as tests/test_match_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the two entry
    points are weak references and stay unresolved.  The file is read and judged before the device is missed, with -g's words and
    exit codes."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_repeat")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f, empty, missing = tmp_path / "in.txt", tmp_path / "empty", tmp_path / "missing"
    f.write_bytes(b"abracadabra" * 100)
    empty.write_bytes(b"")
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, cwd=tmp_path)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        return r

    for dflag in ("", "d"):
        for file in (missing, empty, f):                                 # -g's answer
            a, b = run("-g" + dflag, "abra", file), run("-gk" + dflag, 4, file)
            assert a.returncode == b.returncode != 0 and a.stdout == b.stdout, (file, dflag, b.stdout)
    for K in (0, 32):
        r = run("-gk", K, f)
        assert r.returncode == 253 and "No usable HIP device" in r.stdout
    assert sorted(os.listdir(tmp_path)) == before
