"""CPU: the backward search by byte classes (bce_amd/csrc/class_step.h, what kd_classes.hip runs with a wave per pattern) compiled
by g++ into a stand-alone program under ASan + UBSan, on planes built naively from a BWT made in Python, against a brute force over
the circular text (tests/class_ref.py, itself checked against plain loops): the answers, the node count and the verdict at the
budgets nodes(P) and nodes(P) - 1; the expression language in C++ (class_expr.h) and in Python; the host's linear correction
against a sliding window; the new symbols, names and usage paragraphs, and the CLI's answers without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bce_amd
from bce_amd import api
from conftest import ROOT

import class_ref as ref
import near_ref

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.fixture(scope="module")
def emul():
    exe = os.path.join(ROOT, "tests", "_build", "class_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "class_emul.cpp")])
    return exe


def _hex(b):
    return bytes(b).hex() or "-"


def _mask_hex(masks):
    return _hex(np.ascontiguousarray(masks, dtype="<u4").tobytes())


def _wide(masks):
    return int((np.unpackbits(masks.view(np.uint8), axis=1).sum(axis=1) > 1).sum()) if len(masks) else 0


def test_the_brute_force_is_the_definition():
    """class_ref against three-line loops over the definitions, on texts and patterns small enough for them."""
    rs = np.random.RandomState(5)
    seen = 0
    for t in [b"a", b"ab", b"abab", b"abracadabra", b"\x00\xff" * 5] + [bytes(int(v) for v in rs.randint(0, 3, 17)) for _ in range(4)]:
        n = len(t)
        for masks in ref.cases_for(t):
            m = len(masks)
            sets = [{c for c in range(256) if masks[j][c >> 5] >> (c & 31) & 1} for j in range(m)]
            at = [i for i in range(n) if all(t[(i + j) % n] in sets[j] for j in range(m))]
            assert ref.hits(t, masks).tolist() == at and ref.hits(t, masks).dtype == np.uint32
            assert ref.hits(t, masks, cyclic=False).tolist() == [i for i in at if i + m <= n]
            assert ref.count(t, masks) == len(at) and ref.count(t, masks, cyclic=False) == len([i for i in at if i + m <= n])
            strings = {(j, bytes(t[(i + k) % n] for k in range(j))) for j in range(1, m + 1) for i in range(n)
                       if all(t[(i + k) % n] in sets[m - j + k] for k in range(j))}
            assert ref.nodes(t, masks) == len(strings), (t, m)
            seen += len(strings) > len(at) > 1
    assert seen > 50
    assert ref.exact(b"ab").tolist() == ref.masks_of([[97], [98]]).tolist() and ref.masks_of([ref.ANY]).tolist() == [[0xFFFFFFFF] * 8]


def test_class_search_on_naive_planes_is_the_brute_force(emul, tmp_path):
    """Every pattern at the budgets nodes(P) and nodes(P) - 1.  Within budget: the row intervals expanded through a naive suffix
    array are every hit and none twice, and the node count is nodes(P) exactly; one below: the verdict is `over` with a count
    above the budget.  65 wide classes are refused.  The cases go to the emulator spread over a few processes side by side."""
    texts = near_ref.texts()
    assert len(texts) == 58
    jobs = []                                                            # (cost, text, order, head line, [(masks, budget)])
    for t in texts:
        bwt, row0, order = near_ref.bwt_and_order(t)
        runs = []
        for masks in ref.cases_for(t):
            want = ref.nodes(t, masks)
            runs += [(masks, want)] + ([(masks, want - 1)] if want and _wide(masks) <= 64 else [])
        for at in range(0, len(runs), 16):
            chunk = runs[at:at + 16]
            jobs.append((sum(len(mk) for mk, _ in chunk) + 1, t, order, "%d %d %d\n%s\n" % (len(t), row0, len(chunk), _hex(bwt)), chunk))
    nproc = max(1, min(8, os.cpu_count() or 1))
    bins = [[] for _ in range(nproc)]
    for job in sorted(jobs, key=lambda j: -j[0]):                        # longest first, each to the lightest bin
        min(bins, key=lambda b: sum(j[0] for j in b)).append(job)
    procs = []
    for i, cases in enumerate(bins):
        src = tmp_path / ("cases%d.txt" % i)
        src.write_text("".join(head + "".join("%d %s\n" % (budget, _mask_hex(mk)) for mk, budget in chunk) for _, _, _, head, chunk in cases))
        procs.append(subprocess.Popen([emul, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=SAN_ENV))
    branched = overs = deep = full = 0
    for proc, cases in zip(procs, bins):
        stdout, stderr = proc.communicate()
        assert proc.returncode == 0, (proc.returncode, stderr[-3000:])
        assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
        out = iter(stdout.splitlines())
        for _, t, order, _, chunk in cases:
            order = np.array(order)
            for masks, budget in chunk:
                parts = next(out).split(" | ")
                status, nodes = (int(v) for v in parts[0].split())
                wide = _wide(masks)
                if wide > 64:
                    assert status == 2 and len(parts) == 1, (t, len(masks))
                    deep += 1
                    continue
                want = ref.nodes(t, masks)
                if budget < want:
                    assert status == 1 and nodes > budget, (t, len(masks), budget, nodes)
                    overs += 1
                    continue
                assert status == 0 and nodes == want, (t, len(masks), nodes, want)
                rows = [[int(v) for v in part.split()] for part in parts[1:]]
                assert all(0 <= lo < hi <= len(t) for lo, hi in rows), (t, len(masks))
                pos = np.concatenate([order[lo:hi] for lo, hi in rows] + [np.zeros(0, dtype=np.int64)])
                assert np.array_equal(np.sort(pos), ref.hits(t, masks)), (t, len(masks))       # every hit, and none twice
                branched += len(rows) > 1
                full += wide == 64 and len(rows) > 0
        assert next(out, None) is None
    assert branched > 1000 and overs > 1000 and deep == 58 and full > 20


def test_emulator_refuses_malformed_input(emul, tmp_path):
    one = "00" * 31
    for text in ("3 0 1\n6162\n5 -\n", "2 0 1\n616\n5 -\n", "2 0 2\n6162\n5 -\n", "0 0 0\n-\n", "2 0 1\n6162\n5 %s\n" % one, "2 0 1\n6162\n5\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        r = subprocess.run([emul, str(src)], capture_output=True, text=True, env=SAN_ENV)
        assert r.returncode == 3 and "Sanitizer" not in r.stderr, (text, r.returncode, r.stderr[-2000:])
    src = tmp_path / "bad.txt"
    src.write_text("2 6162\n")
    r = subprocess.run([emul, "--parse", str(src)], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 3 and "Sanitizer" not in r.stderr


# ---- the expression language -------------------------------------------------------------------------------------------------------

GOOD = [b"", b"a", b"abc", b".", b"a.c", b"[abc]", b"[a-c]", b"[a-cx-z0]", b"[^a]", b"[^\\x00]", b"[\\x00-\\x1f]", b"[a\\x7fb]", b"\\x41\\x6a", b"\\\\\\.\\[\\]\\^\\-\\{\\}",
        b"[\\\\\\.\\[\\]\\^\\-\\{\\}]", b"a{3}", b"a{1}", b"[ab]{2}c{3}", b".{4096}", b".{4095}a", b"a{003}", b"[ab]{64}", b"[ab]{65}", b"x[ab]{64}y", b"[.{}[^]",
        b"[a^]", b"^a", b"a-b", b"\xc3\xa9\xff\x80", b"[\xc3\xa9]", b"[\x80-\xff]", b"[^\x80-\xff]", "é[é]".encode("utf-8"), b"[Q-b]", b"[^Q-b]", b"Zz[zA]\\x5a",
        b"[\\x41-\\x5a]", b"\\-{2}", b" \t\n", b"[ -~]{8}"]
BAD = [b"[", b"[a", b"[a-", b"[a-]", b"[-a]", b"[a-b-c]", b"[a--b]", b"[]", b"[^]", b"[b-a]", b"[\\x42-\\x41]", b"]", b"a]", b"{", b"{3}", b"a{", b"a{3", b"a{}", b"a{x}",
       b"a{0}", b"a{4097}", b"a{123456789}", b"a{2}{2}", b"a{-1}", b"}", b"a}", b"\\", b"a\\", b"\\q", b"\\n", b"\\x", b"\\x4", b"\\x4g", b"\\xg4", b"[\\q]", b"[\\x4]",
       b"[a\\", b".{4096}a", b".{4096}.", b"a{4096}b{2}", b".{2049}{2}", b"[a-\\", b"[a-\\q]"]


def test_the_two_parsers_agree_on_every_construct(emul, tmp_path):
    """compile_classes and class_expr.h: the same masks for every expression of a table that holds every construct, with and without
    ignore-case; every malformed expression is refused by both."""
    src = tmp_path / "exprs.txt"
    src.write_text("".join("%d %s\n" % (ic, _hex(e)) for e in GOOD + BAD for ic in (0, 1)))
    r = subprocess.run([emul, "--parse", str(src)], capture_output=True, text=True, env=SAN_ENV)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = iter(r.stdout.splitlines())
    for e in GOOD:
        for ic in (False, True):
            masks = api.compile_classes(e, ignore_case=ic)
            assert masks.dtype == np.uint32 and masks.ndim == 2 and masks.shape[1] == 8
            assert next(out) == "ok " + _mask_hex(masks), (e, ic)
    for e in BAD:
        for ic in (False, True):
            assert next(out) == "bad", (e, ic)
            with pytest.raises(ValueError):
                api.compile_classes(e, ignore_case=ic)
    assert next(out, None) is None
    # what the masks are, for a few of them
    sets = lambda masks: [[c for c in range(256) if masks[j][c >> 5] >> (c & 31) & 1] for j in range(len(masks))]  # noqa: E731
    assert sets(api.compile_classes(b"a.[b-d]")) == [[97], list(range(256)), [98, 99, 100]]
    assert sets(api.compile_classes(b"[^\\x00]")) == [list(range(1, 256))]
    assert sets(api.compile_classes(b"a{3}")) == [[97]] * 3 and api.compile_classes(b".{4096}").shape == (4096, 8)
    assert sets(api.compile_classes(b"a[^b]1", ignore_case=True)) == [[65, 97], [c for c in range(256) if c not in (66, 98)], [49]]
    assert sets(api.compile_classes(b"[Q-b]", ignore_case=True)) == [[65, 66] + list(range(81, 99)) + list(range(113, 123))]
    assert sets(api.compile_classes("é")) == [[0xC3], [0xA9]] and sets(api.compile_classes("é", ignore_case=True)) == [[0xC3], [0xA9]]
    assert sets(api.compile_classes(b"[a\\-c]")) == [[45, 97, 99]] and sets(api.compile_classes(b"\\x41", ignore_case=True)) == [[65, 97]]
    assert api.compile_classes(bytearray(b"ab")).tolist() == api.compile_classes("ab").tolist() == ref.exact(b"ab").tolist()
    assert _wide(api.compile_classes(b"[ab]{64}")) == 64 and _wide(api.compile_classes(b"[ab]{65}")) == 65


def test_linear_correction_turns_cyclic_counts_into_a_sliding_window():
    """cyclic counts less the windows that start in the last m - 1 bytes and match: what a sliding window finds -- texts shorter than
    2 (m - 1), where the two ends overlap, included; zero for m > n; a pattern over budget stays at 0."""
    short = taken = 0
    for t in near_ref.texts():
        n = len(t)
        pats = [p for p in ref.cases_for(t) if len(p)]
        cyc = np.array([ref.count(t, p) for p in pats], dtype=np.uint64)
        got = api.class_linear_counts(cyc, pats, n, lambda e, t=t: (t[:e], t[len(t) - e:]))
        assert got.dtype == np.uint64 and got.shape == (len(pats),)
        for p, g, c in zip(pats, got, cyc):
            m = len(p)
            sets = [{c for c in range(256) if p[j][c >> 5] >> (c & 31) & 1} for j in range(m)] if n < 64 else None
            want = sum(1 for i in range(n - m + 1) if all(t[i + j] in sets[j] for j in range(m))) if sets else ref.count(t, p, cyclic=False)
            assert int(g) == want, (t, m)
            short += 1 < m <= n < 2 * (m - 1)
            taken += int(c) > want
        over = np.arange(len(pats)) % 2 == 0
        again = api.class_linear_counts(cyc, pats, n, lambda e, t=t: (t[:e], t[len(t) - e:]), over)
        assert not again[over].any() and np.array_equal(again[~over], got[~over])
    assert short > 100 and taken > 100


# ---- ABI, names, usage, no-device answers ---------------------------------------------------------------------------------------

NEW = {"bce_hip_count_classes": 8, "bce_hip_count_classes_device": 8, "bce_hip_locate_classes": 11, "bce_hip_locate_classes_device": 11}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    for name, text, value in (("CLASS_MAX_LEN", "4096u", 4096), ("CLASS_MAX_WIDE", "64u", 64), ("CLASS_DEFAULT_NODES", r"\(1u << 16\)", 1 << 16),
                              ("CLASS_MAX_NODES", r"\(1u << 16\)", 1 << 16), ("CLASS_OVER", "1u", 1)):
        assert re.search(r"#define\s+BCE_HIP_%s\s+%s\s*$" % (name, text), src, flags=re.M), name
        assert getattr(api, name) == value, name
    for name in ("CLASS_MAX_LEN", "CLASS_MAX_WIDE", "CLASS_DEFAULT_NODES", "CLASS_MAX_NODES"):
        assert getattr(bce_amd, name) == getattr(api, name)
    for name in ("count_classes", "locate_classes", "compile_classes", "class_linear_counts", "count_classes_tensor", "locate_classes_tensor",
                 "count_classes_in_archive", "locate_classes_in_archive"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("count_classes", "count_classes_device", "locate_classes", "locate_classes_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name
    step = open(os.path.join(ROOT, "bce_amd", "csrc", "class_step.h")).read()
    assert re.search(r"#define\s+BCE_CLASS_MAX_WIDE\s+64u", step) and "kClassExprMax = 4096" in open(os.path.join(ROOT, "bce_amd", "csrc", "class_expr.h")).read()


def test_null_context_is_refused_before_any_device_call():
    lib = bce_amd.load_library()
    masks, off = (C.c_uint32 * 16)(*([1] * 16)), (C.c_uint64 * 2)(0, 2)
    out, work, status = (C.c_uint64 * 2)(7, 7), (C.c_uint64 * 2)(7, 7), (C.c_uint32 * 2)(7, 7)
    total = C.c_uint64(9)
    a = C.addressof
    assert lib.bce_hip_count_classes(None, a(masks), a(off), 1, 0, a(out), a(work), a(status)) == -1
    assert lib.bce_hip_count_classes_device(None, a(masks), a(off), 1, 0, a(out), a(work), a(status)) == -1
    assert lib.bce_hip_count_classes(None, None, None, 0, 0, None, None, None) == -1
    assert lib.bce_hip_locate_classes(None, a(masks), a(off), 1, 0, 0, a(out), a(status), None, 0, C.byref(total)) == -1
    assert lib.bce_hip_locate_classes_device(None, a(masks), a(off), 1, 0, 0, a(out), a(status), None, 0, C.byref(total)) == -1
    assert list(out) == [7, 7] and list(work) == [7, 7] and list(status) == [7, 7] and total.value == 9


HEADS = ["  bce -ge[i] EXPR file", "  bce -ge[i]d EXPR archive.bce", "  bce -ge[i]l EXPR file", "  bce -ge[i]ld EXPR archive.bce"]


def test_usage_has_the_four_paragraphs_and_malformed_command_lines_get_it():
    """In front of `-g`'s paragraph, behind `-gsc`'s: where every older usage test still finds its own."""
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    at = lines.index(HEADS[0])
    assert lines[at - 3] == "  bce -gsc file in.sa" and lines[at - 1] == ""
    assert [lines[at + 3 * i] for i in range(5)] == HEADS + ["  bce -g PATTERN file"]
    assert all(lines[at + 1 + 3 * i].startswith("   ") and lines[at + 2 + 3 * i] == "" for i in range(4))
    assert "{N}" in lines[at + 1] and "\\xHH" in lines[at + 1] and "search gave up" in lines[at + 1] and str(api.CLASS_DEFAULT_NODES) in lines[at + 1]
    for args in (["-ge"], ["-ge", "ab"], ["-ge", "", "file"], ["-ge", "ab", "file", "more"], ["-gex", "ab", "file"], ["-geli", "ab", "file"],
                 ["-gedl", "ab", "file"], ["-geii", "ab", "file"], ["-geild", "ab"], ["-geildd", "ab", "file"], ["-ge", "a[", "file"],
                 ["-gei", "\\q", "file"], ["-gel", "a{0}", "file"], ["-geld", "[]", "file"], ["-ged", ".{4096}a", "file"], ["-ge", "a]", "file"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 0 and "Usage:" in r.stdout, args


def test_sanitized_cli_without_a_device_says_so(tmp_path):
    """The CLI as tests/test_count_cpu.py links it -- CPU only, under ASan + UBSan, tests/asan_stubs.cpp unchanged: the new entry
    points are weak references and stay unresolved.  Files are read and judged before the device is missed, and a malformed EXPR
    before either."""
    exe = os.path.join(ROOT, "tests", "_build", "bce_asan_classes")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = [os.path.join(ROOT, "bce_amd", "csrc", f) for f in ("main.cpp", "decoder.cpp", "host_coder.cpp")] + [os.path.join(ROOT, "tests", "asan_stubs.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe] + src + ["-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    f = tmp_path / "in.txt"
    f.write_bytes(b"abracadabra" * 100)
    before = sorted(os.listdir(tmp_path))
    for cmd in ("-ge", "-gei", "-ged", "-gel", "-geil", "-geld", "-geild"):
        missing = (255, "Archive not found.") if cmd.endswith("d") else (255, "Error loading file")
        for args, (code, text) in (([cmd, "a[bc].{2}\\x61", str(f)], (253, "No usable HIP device")), ([cmd, "[a-c]{3}", str(tmp_path / "missing")], missing),
                                   ([cmd, "a[bc", str(f)], (0, "Usage:")), ([cmd, "a{0}", str(tmp_path / "missing")], (0, "Usage:"))):
            r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, cwd=tmp_path)
            assert r.returncode == code and text in r.stdout, (args, r.returncode, r.stdout)
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == before
