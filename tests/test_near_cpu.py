"""CPU: the branching backward search (bce_amd/csrc/near_step.h, what kd_near.hip runs with a wave per pattern) compiled by g++ into
a stand-alone program under ASan + UBSan, on planes built naively from a BWT made in Python, against a brute force over the
circular text (tests/near_ref.py, itself checked against plain loops); the host's linear correction against a sliding window; the
new symbols, names and usage lines, and the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import near_ref as ref

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def emul():
    exe = os.path.join(ROOT, "tests", "_build", "near_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "near_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def test_the_brute_force_is_the_definition():
    """near_ref against three-line loops over the definition, on texts and patterns small enough for them."""
    rs = np.random.RandomState(5)
    for t in [b"a", b"ab", b"abab", b"abracadabra", b"\x00\xff" * 5] + [bytes(int(v) for v in rs.randint(0, 3, 17)) for _ in range(4)]:
        n = len(t)
        for p in ref.patterns_for(t):
            m = len(p)
            d = [sum(p[j] != t[(i + j) % n] for j in range(m)) for i in range(n)]
            assert ref.distances(t, p).tolist() == d
            for k in (0, 1, 2):
                for cyclic in (True, False):
                    at = [i for i in range(n) if d[i] <= k and (cyclic or i + m <= n)]
                    pos, dist = ref.hits(t, p, k, cyclic)
                    assert pos.dtype == np.uint32 and dist.dtype == np.uint8
                    assert pos.tolist() == at and dist.tolist() == [d[i] for i in at]
                    assert ref.counts(t, p, k, cyclic).tolist() == [sum(1 for i in at if d[i] == e) for e in range(k + 1)]


def test_branching_search_on_naive_planes_is_the_brute_force(emul, tmp_path):
    """Counts per distance, and the (row interval, distance) answers expanded through a naive suffix array, for k = 0, 1, 2.  The
    patterns of a text go to the emulator in chunks, spread over a few processes that run side by side (the long patterns of the
    768-byte text are most of the work)."""
    texts = ref.texts()
    assert len(texts) == 58
    jobs = []                                                            # (cost, text, order, bwt line, patterns)
    for t in texts:
        bwt, row0, order = ref.bwt_and_order(t)
        pats = ref.patterns_for(t)
        for at in range(0, len(pats), 8):
            chunk = pats[at:at + 8]
            jobs.append((sum(len(p) for p in chunk) + 1, t, order, "%d %d %d\n%s\n" % (len(t), row0, len(chunk), _hex(bwt)), chunk))
    nproc = max(1, min(8, os.cpu_count() or 1))
    bins = [[] for _ in range(nproc)]
    for job in sorted(jobs, key=lambda j: -j[0]):                        # longest first, each to the lightest bin
        min(bins, key=lambda b: sum(j[0] for j in b)).append(job)
    procs = []
    for i, cases in enumerate(bins):
        src = tmp_path / ("cases%d.txt" % i)
        src.write_text("".join(head + "\n".join(_hex(p) for p in pats) + "\n" for _, _, _, head, pats in cases))
        procs.append(subprocess.Popen([emul, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=SAN_ENV))
    branched = absent = 0
    for proc, cases in zip(procs, bins):
        stdout, stderr = proc.communicate()
        assert proc.returncode == 0, (proc.returncode, stderr[-3000:])
        assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
        out = iter(stdout.splitlines())
        for _, t, order, _, pats in cases:
            order = np.array(order)
            for p in pats:
                d = ref.distances(t, p)
                for k in (0, 1, 2):
                    parts = next(out).split(" | ")
                    want = np.flatnonzero(d <= k)
                    assert [int(v) for v in parts[0].split()] == np.bincount(d[want], minlength=k + 1)[:k + 1].tolist(), (t, p, k)
                    rows = [[int(v) for v in part.split()] for part in parts[1:]]
                    assert all(0 <= lo < hi <= len(t) and e <= k for lo, hi, e in rows), (t, p, k)
                    pos = np.concatenate([order[lo:hi] for lo, hi, _ in rows] + [np.zeros(0, dtype=np.int64)])
                    dist = np.concatenate([np.full(hi - lo, e) for lo, hi, e in rows] + [np.zeros(0, dtype=np.int64)])
                    by_pos = np.argsort(pos, kind="stable")
                    assert np.array_equal(pos[by_pos], want), (t, p, k)                # every hit, and none twice
                    assert np.array_equal(dist[by_pos], d[want]), (t, p, k)
                    branched += len(rows) > 1
                absent += bool(p) and p[-1] not in t and int((d <= 1).sum()) > 0
        assert next(out, None) is None
    assert branched > 1000 and absent > 20          # many intervals per answer; a last byte the text lacks, found at distance 1


def test_emulator_refuses_malformed_input(emul, tmp_path):
    for text in ("3 0 1\n6162\n61\n", "2 0 1\n616\n61\n", "2 0 2\n6162\n61\n", "0 0 0\n-\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])


def test_linear_correction_turns_cyclic_counts_into_a_sliding_window():
    """cyclic counts per distance, less the windows that start in the last m - 1 bytes: what a sliding window finds -- texts shorter
    than 2 (m - 1), where the two ends overlap, included; zeros for m > n."""
    short = 0
    for t in ref.texts():
        n = len(t)
        pats = [p for p in ref.patterns_for(t) if p]
        for k in (0, 1, 2):
            cyc = np.array([ref.counts(t, p, k) for p in pats], dtype=np.uint64)
            got = api.near_linear_counts(cyc, pats, n, lambda e, t=t: (t[:e], t[len(t) - e:]))
            assert got.dtype == np.uint64 and got.shape == (len(pats), k + 1)
            for p, g in zip(pats, got):
                m = len(p)
                want = [sum(1 for i in range(n - m + 1) if sum(a != b for a, b in zip(p, t[i:i + m])) == e) for e in range(k + 1)] if n < 64 else \
                    ref.counts(t, p, k, cyclic=False).tolist()
                assert g.tolist() == want, (t, p, k)
                short += 1 < m <= n < 2 * (m - 1)
    assert short > 100


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_count_near": 6, "bce_hip_count_near_device": 6, "bce_hip_locate_near": 11, "bce_hip_locate_near_device": 11}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"#define\s+BCE_HIP_NEAR_MAX_K\s+2u", src) and re.search(r"#define\s+BCE_HIP_NEAR_MAX_LEN\s+4096u", src)
    assert api.NEAR_MAX_K == 2 and api.NEAR_MAX_LEN == 4096
    for name in ("count_near", "locate_near", "count_near_tensor", "locate_near_tensor", "count_near_in_archive", "locate_near_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("count_near", "count_near_device", "locate_near", "locate_near_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name


def test_null_context_is_refused_before_any_device_call():
    lib = bce_amd.load_library()
    pat, off, out = (C.c_uint8 * 4)(97, 98, 99, 100), (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 3)(7, 7, 7)
    total = C.c_uint64(9)
    a = C.addressof
    assert lib.bce_hip_count_near(None, a(pat), a(off), 1, 1, a(out)) == -1
    assert lib.bce_hip_count_near_device(None, a(pat), a(off), 1, 1, a(out)) == -1
    assert lib.bce_hip_count_near(None, None, None, 0, 0, None) == -1
    assert lib.bce_hip_locate_near(None, a(pat), a(off), 1, 1, 0, a(out), None, None, 0, C.byref(total)) == -1
    assert lib.bce_hip_locate_near_device(None, a(pat), a(off), 1, 1, 0, a(out), None, None, 0, C.byref(total)) == -1
    assert list(out) == [7, 7, 7] and total.value == 9


def test_usage_has_the_four_lines_directly_after_the_locate_paragraph():
    """Directly after `-gl`'s paragraph; `-gld` follows them, with `-gm` behind it as before."""
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    at = lines.index("  bce -gl PATTERN file")
    assert lines[at + 1].startswith("   ") and lines[at + 2] == ""
    assert [lines[at + 3 + 3 * i] for i in range(5)] == ["  bce -gn K PATTERN file", "  bce -gnd K PATTERN archive.bce", "  bce -gnl K PATTERN file",
                                                        "  bce -gnld K PATTERN archive.bce", "  bce -gld PATTERN archive.bce"]
    assert all(lines[at + 4 + 3 * i].startswith("   ") and lines[at + 5 + 3 * i] == "" for i in range(5))
    assert "0..2" in lines[at + 4] and lines[at + 18] == "  bce -gm MINLEN file query_file"
    for args in (["-gn"], ["-gn", "1"], ["-gn", "1", "ab"], ["-gn", "3", "ab", "file"], ["-gn", "x", "ab", "file"], ["-gnx", "1", "ab", "file"],
                 ["-gn", "1", "", "file"], ["-gn", "-1", "ab", "file"], ["-gn", "01", "ab", "file"], ["-gn", "", "ab", "file"], ["-gnd", "1", "ab", "a", "b"],
                 ["-gnl", "3", "ab", "file"], ["-gnl", "1", "ab"], ["-gnld", "2", "", "file"], ["-gnlx", "1", "ab", "file"], ["-gnld", "1", "ab", "a", "b"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_without_a_device_says_so(tmp_path):
    """The CLI as tests/test_count_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the new entry
    points are weak references and stay unresolved.  Files are read and judged before the device is missed."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_near")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f = tmp_path / "in.txt"
    f.write_bytes(b"abracadabra" * 100)
    before = sorted(os.listdir(tmp_path))
    for cmd in ("-gn", "-gnd", "-gnl", "-gnld"):
        missing = (255, "Archive not found.") if cmd.endswith("d") else (255, "Error loading file")
        for args, (code, text) in (([cmd, "1", "abra", str(f)], (253, "No usable HIP device")), ([cmd, "2", "abra", str(tmp_path / "missing")], missing)):
            r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, cwd=tmp_path)
            assert r.returncode == code and text in r.stdout, (args, r.returncode, r.stdout)
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == before
