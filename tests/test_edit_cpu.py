"""CPU: the three-way branching backward search (bce_amd/csrc/edit_step.h, what kd_edit.hip runs with a wave per pattern) compiled by
g++ into a stand-alone program under ASan + UBSan, on planes built naively from a BWT made in Python: its candidates, expanded through
a naive suffix array and reduced to the least (distance, length) per position, against the definition (tests/edit_ref.py, itself
checked against plain loops); the conditions the GPU tests put on their inputs; the new symbols, names and usage lines, and the CLI's
answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import edit_ref as ref
import near_ref

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def emul():
    exe = os.path.join(ROOT, "tests", "_build", "edit_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "edit_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _triples(h):
    return list(zip(h[0].tolist(), h[1].tolist(), h[2].tolist()))


def test_the_table_is_the_definition():
    """edit_ref's banded DP against plain loops over the definition, on texts of 12 bytes and less: every k, both modes."""
    rs = np.random.RandomState(7)
    texts = [b"a", b"ab", b"abab", b"aaaa", b"abracadabra"] + [bytes(int(v) for v in rs.randint(0, s, n)) for s, n in ((1, 5), (2, 9), (2, 12), (3, 12), (3, 7), (2, 3))]
    indel = 0
    for t in texts:
        for p in ref.patterns_for(t):
            E = ref.table(t, p)
            for k in (0, 1, 2):
                for cyclic in (True, False):
                    want = ref.hits_by_loops(t, p, k, cyclic)
                    got = ref.hits_of(E, len(p), len(t), k, cyclic)
                    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint16 and got[2].dtype == np.uint8
                    assert _triples(got) == want, (t, p, k, cyclic)
                    assert ref.counts(t, p, k, cyclic).tolist() == [sum(1 for v in want if v[2] == e) for e in range(k + 1)]
                    indel += sum(1 for v in want if v[1] != len(p))
    assert indel > 1000
    assert ref.anchored(b"colour", b"color") == 1 and ref.anchored(b"abc", b"xabc") == 2 and ref.anchored(b"ab", b"axb") == 1
    assert ref.anchored(b"", b"") == 0 and ref.anchored(b"", b"a") is None and ref.anchored(b"a", b"ab") is None and ref.anchored(b"ab", b"a") is None


def test_branching_search_on_naive_planes_reduces_to_the_definition(emul, tmp_path):
    """Every candidate (row interval, distance, length) expanded through a naive suffix array; per position the least (distance,
    length), in linear mode among the candidates that end inside the text: the definition's hits for k = 0, 1, 2.  The patterns of a
    text go to the emulator in chunks, spread over a few processes that run side by side."""
    texts = near_ref.texts()
    assert len(texts) == 58
    jobs = []                                                            # (cost, text, order, bwt line, patterns)
    for t in texts:
        bwt, row0, order = near_ref.bwt_and_order(t)
        pats = ref.patterns_for(t)
        for at in range(0, len(pats), 4):                                # (a node's cost grows with the bytes that can precede it)
            chunk = pats[at:at + 4]
            jobs.append(((sum(len(p) for p in chunk) + 1) * len(set(t)), t, order, "%d %d %d\n%s\n" % (len(t), row0, len(chunk), _hex(bwt)), chunk))
    nproc = max(1, min(8, os.cpu_count() or 1))
    bins = [[] for _ in range(nproc)]
    for job in sorted(jobs, key=lambda j: -j[0]):                        # longest first, each to the lightest bin
        min(bins, key=lambda b: sum(j[0] for j in b)).append(job)
    procs = []
    for i, cases in enumerate(bins):
        src = tmp_path / ("cases%d.txt" % i)
        src.write_text("".join(head + "\n".join(_hex(p) for p in pats) + "\n" for _, _, _, head, pats in cases))
        procs.append(subprocess.Popen([emul, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=SAN_ENV))
    many = nested = shorter = longer = 0
    for proc, cases in zip(procs, bins):
        stdout, stderr = proc.communicate()
        assert proc.returncode == 0, (proc.returncode, stderr[-3000:])
        assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
        out = iter(stdout.splitlines())
        for _, t, order, _, pats in cases:
            order, n = np.array(order, dtype=np.int64), len(t)
            for p in pats:
                E, m = ref.table(t, p), len(p)
                for k in (0, 1, 2):
                    parts = next(out).split(" | ")
                    rows = np.array([[int(v) for v in part.split()] for part in parts[1:]], dtype=np.int64).reshape(-1, 4)
                    assert int(parts[0]) == len(rows)
                    assert ((0 <= rows[:, 0]) & (rows[:, 0] < rows[:, 1]) & (rows[:, 1] <= n) & (rows[:, 2] <= k)).all(), (t, p, k)
                    assert ((rows[:, 3] >= max(0, m - k)) & (rows[:, 3] <= m + k)).all(), (t, p, k)
                    width = rows[:, 1] - rows[:, 0]
                    pos = np.concatenate([order[lo:hi] for lo, hi in rows[:, :2]] + [np.zeros(0, dtype=np.int64)])
                    key = np.repeat(rows[:, 2] * 8192 + rows[:, 3], width)
                    length = np.repeat(rows[:, 3], width)
                    for cyclic in (True, False):
                        live = np.ones(len(pos), dtype=bool) if cyclic else pos + length <= n
                        best = np.full(n, 1 << 40, dtype=np.int64)
                        np.minimum.at(best, pos[live], key[live])
                        at = np.flatnonzero(best < 1 << 40)
                        want = ref.hits_of(E, m, n, k, cyclic)
                        assert np.array_equal(at, want[0]) and np.array_equal(best[at] % 8192, want[1]) and np.array_equal(best[at] // 8192, want[2]), (t, p, k, cyclic)
                    many += len(pos) > len(np.unique(pos))
                    nested += len(np.unique(rows[:, 3])) >= 3
                    hit = ref.hits_of(E, m, n, k, True)
                    shorter += int((hit[1] < m).sum())
                    longer += int((hit[1] > m).sum())
        assert next(out, None) is None
    # positions found more than once, candidates at three lengths and more, hits through deletions and through insertions
    assert many > 1000 and nested > 1000 and shorter > 1000 and longer > 1000


def test_emulator_refuses_malformed_input(emul, tmp_path):
    for text in ("3 0 1\n6162\n61\n", "2 0 1\n616\n61\n", "2 0 2\n6162\n61\n", "0 0 0\n-\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


def test_the_gpu_tests_inputs_are_what_they_are_chosen_for():
    """The conditions tests/test_gpu_edit.py relies on, from the definition alone."""
    text, pats = ref.four_case()
    assert len(text) == 1 << 16 and len(pats) == 100 and min(len(p) for p in pats) == 3 and max(len(p) for p in pats) >= 24
    assert len({len(p) for p in pats[:4]}) > 1                          # lengths differ within a workgroup
    tables = [ref.table(text, p) for p in pats]
    assert max(int(ref.candidate_lengths(E, 2).max()) for E in tables) >= 3
    hits = [ref.hits_of(E, len(p), len(text), 2) for E, p in zip(tables, pats)]
    assert sum(len(h[0]) for h in hits) > 50000 and sum(int((h[1] != len(p)).sum()) for h, p in zip(hits, pats)) > 1000
    text, pats = ref.random_case()
    assert len(text) == 1 << 20 and len(pats) == 64 and all(len(p) == 8 for p in pats)
    tables = [ref.table(text, p) for p in pats]
    assert sum(len(ref.hits_of(E, 8, len(text), 0)[0]) for E in tables) < 8
    for cyclic in (True, False):
        hits = [ref.hits_of(E, 8, len(text), 2, cyclic) for E in tables]
        assert sum(len(h[0]) for h in hits) >= 8 and sum(int((h[1] != 8).sum()) for h in hits) >= 4
    text, pats = ref.scan_case()
    assert len(pats) == 2100 > 2048
    got = [len(ref.hits(text, p, 1, cyclic)[0]) for p in pats[:6] for cyclic in (True, False)]
    assert got[0] > 10000 and got[1] > 10000 and got[2:6] == [0, 0, 0, 0] and got[10:] == [0, 0]
    text, p = ref.linear_case()
    n = len(text)
    assert text.endswith(b"abc") and text.startswith(b"d") and p == b"abcd"
    assert (n - 3, 4, 0) in _triples(ref.hits(text, p, 2, True)) and (n - 3, 3, 2) in _triples(ref.hits(text, p, 2, False))


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_count_edit": 7, "bce_hip_count_edit_device": 7, "bce_hip_locate_edit": 12, "bce_hip_locate_edit_device": 12}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"#define\s+BCE_HIP_EDIT_MAX_K\s+2u", src) and re.search(r"#define\s+BCE_HIP_EDIT_MAX_LEN\s+4096u", src)
    assert re.search(r"#define\s+BCE_HIP_EDIT_MAX_PATTERNS\s+\(1u << 28\)", src)
    assert api.EDIT_MAX_K == 2 and api.EDIT_MAX_LEN == 4096 and api.EDIT_MAX_PATTERNS == 1 << 28 >= 1 << 24
    step = open(os.path.join(ROOT, "bce_amd", "csrc", "edit_step.h")).read()
    assert re.search(r"#define\s+BCE_EDIT_MAX_K\s+2u", step) and re.search(r"#define\s+BCE_EDIT_CODE_BITS\s+4u", step)
    for name in ("count_edit", "locate_edit", "count_edit_tensor", "locate_edit_tensor", "count_edit_in_archive", "locate_edit_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("count_edit", "count_edit_device", "locate_edit", "locate_edit_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name


def test_null_context_is_refused_before_any_device_call():
    lib = bce_amd.load_library()
    pat, off, out = (C.c_uint8 * 4)(97, 98, 99, 100), (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 3)(7, 7, 7)
    total = C.c_uint64(9)
    a = C.addressof
    assert lib.bce_hip_count_edit(None, a(pat), a(off), 1, 1, 0, a(out)) == -1
    assert lib.bce_hip_count_edit_device(None, a(pat), a(off), 1, 1, 0, a(out)) == -1
    assert lib.bce_hip_count_edit(None, None, None, 0, 0, 0, None) == -1
    assert lib.bce_hip_locate_edit(None, a(pat), a(off), 1, 1, 0, a(out), None, None, None, 0, C.byref(total)) == -1
    assert lib.bce_hip_locate_edit_device(None, a(pat), a(off), 1, 1, 0, a(out), None, None, None, 0, C.byref(total)) == -1
    assert list(out) == [7, 7, 7] and total.value == 9


def test_usage_has_the_four_lines_between_the_estimate_and_the_repeats():
    """Directly after `-e`'s paragraph and before `-gp`'s; `-gf` / `-gfd` stay last."""
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    at = lines.index("  bce -e file [config.bcc]")
    assert lines[at + 1].startswith("   ") and lines[at + 2] == ""
    assert [lines[at + 3 + 3 * i] for i in range(5)] == ["  bce -gw K PATTERN file", "  bce -gwd K PATTERN archive.bce", "  bce -gwl K PATTERN file",
                                                        "  bce -gwld K PATTERN archive.bce", "  bce -gp ORDER MINLEN N file"]
    assert all(lines[at + 4 + 3 * i].startswith("   ") and lines[at + 5 + 3 * i] == "" for i in range(5))
    assert "0..2" in lines[at + 4] and "POS LEN d" in lines[at + 10] and lines[-1].startswith("   ") and lines[-2] == "  bce -gfd K N archive.bce"
    for args in (["-gw"], ["-gw", "1"], ["-gw", "1", "ab"], ["-gw", "3", "ab", "file"], ["-gw", "x", "ab", "file"], ["-gwx", "1", "ab", "file"],
                 ["-gw", "1", "", "file"], ["-gw", "-1", "ab", "file"], ["-gw", "01", "ab", "file"], ["-gw", "", "ab", "file"], ["-gwd", "1", "ab", "a", "b"],
                 ["-gwl", "3", "ab", "file"], ["-gwl", "1", "ab"], ["-gwld", "2", "", "file"], ["-gwlx", "1", "ab", "file"], ["-gwld", "1", "ab", "a", "b"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_without_a_device_says_so(tmp_path):
    """The CLI as tests/test_count_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the new entry
    points are weak references and stay unresolved.  Files are read and judged before the device is missed."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_edit")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f = tmp_path / "in.txt"
    f.write_bytes(b"abracadabra" * 100)
    before = sorted(os.listdir(tmp_path))
    for cmd in ("-gw", "-gwd", "-gwl", "-gwld"):
        missing = (255, "Archive not found.") if cmd.endswith("d") else (255, "Error loading file")
        for args, (code, text) in (([cmd, "1", "abra", str(f)], (253, "No usable HIP device")), ([cmd, "2", "abra", str(tmp_path / "missing")], missing)):
            r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, cwd=tmp_path)
            assert r.returncode == code and text in r.stdout, (args, r.returncode, r.stdout)
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == before
